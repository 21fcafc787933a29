"""Drop-in for the reference's sparse descriptor loss (superpoint/loss_functions/sparse_loss.py:98-174): the same signatures and
return tuples, forward VALUE only.  The cell warp, the compaction, the gathers and every product run in libimx
(imx_desc_loss_sparse); the random draws are restated on the device (image_matching_amd.sptrain: their own stream, unpinned).
Differences, all documented in INTEGRATION.md: tensors stay on the device and nothing is read back, so an image with no valid
cell yields NaN losses where the reference raises inside np.random.choice; only dist='cos' is served."""
import torch

from ... import sptrain


def _check(dist, method):
    if dist != 'cos':
        raise NotImplementedError(f"descriptor_loss_sparse: only dist='cos' (the shipped yaml) is served, got {dist!r}")
    if method not in ('1d', '2d'):
        raise ValueError(f"descriptor_loss_sparse: method must be '1d' or '2d', got {method!r}")


def _batch(descriptors, descriptors_warped, homographies, lamda_d, num_matching_attempts, num_masked_non_matches_per_match, method):
    B, d, Hc, Wc = descriptors.shape
    eng = sptrain.plain_engine(descriptors.device, d)
    hom = homographies.type(torch.float32).reshape(B, 3, 3)
    choice, non = sptrain.draw(eng, hom, Hc, Wc, int(num_matching_attempts), int(num_masked_non_matches_per_match))
    return eng.desc_loss_sparse(descriptors, descriptors_warped, hom, choice, non, lamda_d=lamda_d, margin=0.2, method=method)


def descriptor_loss_sparse(descriptors, descriptors_warped, homographies, mask_valid=None,
                           cell_size=8, device='cpu', descriptor_dist=4, lamda_d=250,
                           num_matching_attempts=1000, num_masked_non_matches_per_match=10,
                           dist='cos', method='1d', **config):
    """descriptors, descriptors_warped [D, Hc, Wc] on the GPU -> (loss, lamda_d * match_loss, non_match_loss), 0-d device tensors."""
    _check(dist, method)
    out = _batch(descriptors[None], descriptors_warped[None], homographies, lamda_d, num_matching_attempts,
                 num_masked_non_matches_per_match, method)["out"][0]
    return out[0], out[1], out[2]


def batch_descriptor_loss_sparse(descriptors, descriptors_warped, homographies, **options):
    """The reference's batch loop as one launch sequence: (loss.mean(), None, pos_loss.mean(), neg_loss.mean())."""
    _check(options.get('dist', 'cos'), options.get('method', '1d'))
    mean = _batch(descriptors, descriptors_warped, homographies, options.get('lamda_d', 250), options.get('num_matching_attempts', 1000),
                  options.get('num_masked_non_matches_per_match', 10), options.get('method', '1d'))["mean"]
    return mean[0], None, mean[1], mean[2]
