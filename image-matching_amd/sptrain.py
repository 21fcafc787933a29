"""SuperPoint descriptor training (the reference's superpoint_train_descriptor.py -> datasets/ALLSS.py ->
superpoint/Train_model_heatmap.py:83-314), host plumbing: the random draws of the sparse descriptor loss restated with torch ops on
the device, and the handle the weight-free stages share.  All arithmetic on maps and descriptors runs in libimx (csrc/sptrain.hip).

The draws are valid samples of the reference's distributions but NOT its stream (it draws from numpy's and torch's global CPU
generators): unpinned, like the homography sampler.  The kernels take indices, so a caller can inject any draws -- the tests inject
the reference's own."""
import torch

from .engine import Engine

_engines = {}


def plain_engine(device, d=256):
    """A handle without weights, for the stages that need none (labels, masks, both losses); one per (device, d)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"image_matching_amd runs on 'cuda' (HIP) devices only, got {device!r}; there is no CPU fallback")
    dev = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
    key = (str(dev), int(d))
    if key not in _engines:
        _engines[key] = Engine({"descriptor_dim": int(d)}, {"descriptor_dim": int(d)}, dev)
    return _engines[key]


def draw_choice(n_valid, M, cells, generator=None):
    """crop_or_pad_choice(n_valid, M, shuffle=True) (utils/utils.py:334-356) for B images without reading n_valid back: a random
    permutation of [0, n_valid), its first M entries, padded -- where n_valid < M -- with uniform draws (with replacement) from it.
    n_valid (B) int32 device tensor, cells = Hc Wc >= every n_valid.  Returns (B,M) int32.  n_valid = 0 yields index 0, which
    imx_desc_loss_sparse answers with NaN losses for that image (the reference raises inside np.random.choice)."""
    dev = n_valid.device
    B = n_valid.numel()
    nv = n_valid.to(torch.int64).view(B, 1)
    keys = torch.rand(B, cells, device=dev, generator=generator)
    keys = torch.where(torch.arange(cells, device=dev)[None] < nv, keys, torch.full_like(keys, 2.0))
    perm = torch.argsort(keys, dim=1)                                   # the first n_valid entries: a permutation of the valid indices
    m = torch.arange(M, device=dev)[None].expand(B, M)
    pad = (torch.rand(B, M, device=dev, generator=generator) * nv).floor().to(torch.int64)
    pad = torch.minimum(pad, torch.clamp(nv - 1, min=0))
    pos = torch.where(m < nv, m, pad)
    pos = torch.clamp(pos, max=cells - 1)
    return torch.gather(perm, 1, pos).to(torch.int32).contiguous()


def draw_non_matches(pairs, choice, Hc, Wc, R, generator=None):
    """create_non_correspondences (superpoint/correspondence_tools/correspondence_finder.py:191-320) and the reference's way to a flat
    index, (u + v Wc) in float then .long() (sparse_loss.py:57-61, :93-94), for B images: R uniform cells per match; a draw within one
    cell of its match in u or v is moved by the same normal(+-0.5, 10) offset in both coordinates; one wrap by (size - 1).  A result
    that still leaves the map -- where the reference's index_select raises -- is clamped into it.  pairs (B,Hc Wc,2) int32 from
    Engine.desc_pairs, choice (B,M) int32.  Returns (B,M,R) int32."""
    dev = pairs.device
    B, M = choice.shape
    b_cell = torch.gather(pairs[..., 1].to(torch.int64), 1, choice.to(torch.int64)).clamp(min=0)
    ub, vb = (b_cell % Wc).float()[..., None], (b_cell // Wc).float()[..., None]
    u = (torch.rand(B, M, R, device=dev, generator=generator) * Wc).floor()
    v = (torch.rand(B, M, R, device=dev, generator=generator) * Hc).floor()
    close = (((ub - u).abs() < 1.0) | ((vb - v).abs() < 1.0)).float()
    minimal = (torch.rand(B, M, R, device=dev, generator=generator) * 2).floor() * 1.0 - 0.5
    perturb = close * (torch.randn(B, M, R, device=dev, generator=generator) * 10 + minimal)
    u, v = u + perturb, v + perturb
    for c, size in ((u, Wc), (v, Hc)):
        hi = float(size) - 1
        c.copy_(torch.where(c > hi, c - hi, c))
        c.copy_(torch.where(c < 0.0, c + hi, c))
    flat = (u + v * Wc).long()
    return flat.clamp(0, Hc * Wc - 1).to(torch.int32).contiguous()


def draw(engine, homographies, Hc, Wc, M, R, generator=None):
    """Both draws for a batch: (choice (B,M), nonmatch_b (B,M,R)) int32 device tensors, no host synchronisation."""
    pairs, n_valid = engine.desc_pairs(homographies, Hc, Wc)
    choice = draw_choice(n_valid, M, Hc * Wc, generator)
    return choice, draw_non_matches(pairs, choice, Hc, Wc, R, generator)
