/* imx_mhagrad.h -- C ABI of libimx_mhagrad.so, the fifth library on libimx.so's handles (include/imx.h; beside imx_sptrain.h,
 * imx_spgrad.h and imx_otgrad.h): the attention of SuperGlue's GNN (superglue/models/superglue_train.py:82-86: einsum, softmax, einsum)
 * in its training form -- a forward that keeps the row log-sum-exp instead of the probabilities, and the backward that recomputes them.
 * Per (pair b, head h), with D the head dimension and scale = 1 / sqrt(D) (the reference's dim ** .5, dim = query.shape[1]):
 *
 *   forward    S = scale Q^T K (n_q x n_k),  P = softmax_rows(S),  O = P V,  lse_i = log sum_j exp(S_ij)
 *   backward   delta_i = sum_c dO_ic O_ic,  P = exp(S - lse) (recomputed, never stored),
 *              dV = P^T dO,  dP = dO V^T,  dS = P o (dP - delta) scale,  dQ = dS K,  dK = dS^T Q
 *
 * Layout: the reference's own tensors, read and written in place: (B, D, H, n) contiguous fp32, element (b, c, h, n) at
 * ((b D + c) H + h) n_frame + n, which is what conv1d(...).view(B, dim, heads, -1) yields (no copy, no permute); q, out, dout and dq
 * over a frame of N queries, k, v, dk and dv over a frame of M keys.  lse is (B, H, N).  No alignment beyond 4 bytes is assumed.
 *
 * Ragged batches: n_q = nq_dev[b], n_k = nk_dev[b] are read on the device (NULL = N / M; clamped to [0,N] / [0,M]).  Queries past n_q and
 * keys past n_k are never read and may hold anything, NaN included.  out, lse, dq, dk and dv are written in full, with 0 there; n_q = 0 or
 * n_k = 0 gives zeros everywhere for that pair.
 *
 * Arithmetic: every product on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32), fp32 accumulation; a tile's 32 terms accumulate from
 * zero and are then added to the running sum (two levels).  No floating-point atomics, no workgroup that waits on another, no
 * cooperative launch: the order of every sum is fixed at compile time and depends on the pair's own counts only, so equal inputs give
 * equal bits between calls, handles, batch compositions, paddings and workspace histories.
 *
 * Built with the other four from one source tree (image-matching_amd/csrc/Makefile); use all from the SAME build.  The calls take an
 * imx_handle_t that libimx.so's imx_create made, draw their scratch from that handle's workspace ("mha.delta": B H N floats, written by
 * the backward call that reads it; nothing of size N M), report errors through imx_last_error and timing rows through
 * imx_timing_report, and follow the conventions at the top of imx.h.  A library of its own because the symbol tables of the other four
 * are pinned.  Asynchronous on the caller's stream, no host read.
 *
 * Not here: the q / k / v projections, the merge, the MLP and their backward (the caller's framework runs them), dropout, masks other
 * than the counts, the 16-bit plane forms of the inference path, a second derivative.
 */
#ifndef IMX_MHAGRAD_H
#define IMX_MHAGRAD_H

#include "imx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* q (B,D,H,N), k and v (B,D,H,M) -> out (B,D,H,N), lse (B,H,N).  lse_dev may be NULL (value only).
 * 1 <= B H <= 65535, 1 <= N, M <= 2^20, D in {16, 32, 64}: anything else, or a null q / k / v / out, returns an error code, sets
 * imx_last_error and launches nothing. */
IMX_API int imx_mha_forward_train(imx_handle_t h, int B, int H, int D, int N, int M,
                                  const float* q_dev, const float* k_dev, const float* v_dev,
                                  const int32_t* nq_dev, const int32_t* nk_dev,
                                  float* out_dev, float* lse_dev, void* stream);

/* the same q, k, v, the forward's out and lse, dout (B,D,H,N) -> dq (B,D,H,N), dk, dv (B,D,H,M).
 * Any of dq_dev / dk_dev / dv_dev may be NULL: that gradient is not formed (dq NULL skips the per-query kernel, dk and dv both NULL the
 * per-key kernel); the others keep their bits.  The same bounds and error rules; q, k, v, out, lse and dout are required. */
IMX_API int imx_mha_backward(imx_handle_t h, int B, int H, int D, int N, int M,
                             const float* q_dev, const float* k_dev, const float* v_dev,
                             const float* out_dev, const float* lse_dev, const float* dout_dev,
                             const int32_t* nq_dev, const int32_t* nk_dev,
                             float* dq_dev, float* dk_dev, float* dv_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMX_MHAGRAD_H */
