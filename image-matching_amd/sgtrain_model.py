"""A trainable SuperGlue: the reference's training model (superglue/models/superglue_train.py:174-307) as a torch.nn.Module with live
parameters whose training forward AND backward run in the libraries -- every convolution, BatchNorm + ReLU, attention, the score product
and the match loss through image_matching_amd.sgtrain_grad (include/imx_train.h, include/imx_sgtrain.h); PyTorch does the keypoint
normalisation, the residual adds and the optimiser step.

    engine = Engine(None, config, "cuda")
    model = SuperGlueTrainable(config, engine).train()
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-4)
    out = model(sample, want_matches=False)          # one GlueSparse / Engine.train_pairs sample, the reference's dict
    if not out['skip_train']:
        optimizer.zero_grad()
        out['loss'].backward()
        optimizer.step()

The modules are plain nn.Conv1d / nn.BatchNorm1d / nn.ReLU containers in the reference's layout, so state_dict() has exactly the keys
and shapes of the reference's checkpoints (synth.superglue_shapes): a checkpoint of the reference loads here, and this model's
state_dict loads into the inference SuperGlue of superglue/models/superglue_test.py.  The drop-in superglue_train.SuperGlue stays the
evaluation-only class it was.

The loss of a batch: the reference trains with batch size 1.  forward_pairs() returns the per-pair loss (B) of a padded batch of pairs
with different keypoint counts; the loss of the batch is, by definition here, forward_pairs(...).mean().  With counts the BatchNorm
statistics of each call are those of the valid columns of all pairs (include/imx_train.h)."""
from collections.abc import Mapping

import torch
from torch import nn

from . import sgtrain_grad as G
from .engine import ImxError

DEFAULT_CONFIG = {                      # superglue_train.py:192-199
    'descriptor_dim': 256,
    'weights': '',
    'keypoint_encoder': [32, 64, 128, 256],
    'GNN_layers': ['self', 'cross'] * 9,
    'sinkhorn_iterations': 100,
    'match_threshold': 0.2,
}
HEADS = 4                               # AttentionalPropagation(feature_dim, 4), superglue_train.py:123


def _mlp(channels):
    """Conv1d(kernel_size=1) [BatchNorm1d ReLU Conv1d] ... over `channels`, the last bias 0"""
    mods = []
    for i in range(1, len(channels)):
        mods.append(nn.Conv1d(channels[i - 1], channels[i], kernel_size=1, bias=True))
        if i < len(channels) - 1:
            mods += [nn.BatchNorm1d(channels[i]), nn.ReLU()]
    nn.init.constant_(mods[-1].bias, 0.0)
    return nn.Sequential(*mods)


class _Attention(nn.Module):
    """the parameters of MultiHeadedAttention: merge and the three projections, which start as copies of merge"""

    def __init__(self, num_heads, d_model):
        super().__init__()
        self.dim, self.num_heads = d_model // num_heads, num_heads
        self.merge = nn.Conv1d(d_model, d_model, kernel_size=1)
        self.proj = nn.ModuleList([nn.Conv1d(d_model, d_model, kernel_size=1) for _ in range(3)])
        for p in self.proj:
            p.load_state_dict(self.merge.state_dict())


class _Propagation(nn.Module):
    """the parameters of AttentionalPropagation: .attn and .mlp, what sgtrain_grad.gnn_layer takes"""

    def __init__(self, feature_dim, num_heads):
        super().__init__()
        self.attn = _Attention(num_heads, feature_dim)
        self.mlp = _mlp([2 * feature_dim, 2 * feature_dim, feature_dim])


class _Encoder(nn.Module):
    def __init__(self, feature_dim, layers):
        super().__init__()
        self.encoder = _mlp([3] + list(layers) + [feature_dim])


class _Gnn(nn.Module):
    def __init__(self, feature_dim, layer_names):
        super().__init__()
        self.layers = nn.ModuleList([_Propagation(feature_dim, HEADS) for _ in layer_names])
        self.names = list(layer_names)


def build_modules(config):
    """(kenc, gnn, final_proj) for a merged config: containers of parameters only, in the reference's layout and with its initialisation
    (PyTorch's defaults; the last bias of the keypoint encoder and of every MLP 0).  No GPU is needed."""
    d = int(config['descriptor_dim'])
    if d % HEADS or d // HEADS not in (16, 32, 64):
        raise ImxError(f"SuperGlueTrainable: descriptor_dim / {HEADS} must be 16, 32 or 64 (the head dimensions of imx_mha_forward_train), "
                       f"got descriptor_dim = {d}")
    return _Encoder(d, config['keypoint_encoder']), _Gnn(d, config['GNN_layers']), nn.Conv1d(d, d, kernel_size=1, bias=True)


def normalize_keypoints(kpts, image_shape):
    """(kpts - (W, H) / 2) / (0.7 max(W, H)) for kpts (B,N,2) in pixels and image_shape (.., H, W) (superglue_train.py:60-67)"""
    height, width = image_shape[-2:]
    size = kpts.new_tensor([float(width), float(height)])
    return (kpts - size / 2) / (0.7 * size.max())


def transport(scores, bin_score, iters):
    """log_optimal_transport (superglue_train.py:138-167) restated for scores (B,m,n): the (B,m+1,n+1) log-assignment after `iters`
    Sinkhorn half-iteration pairs in the log domain, times m + n"""
    b, m, n = scores.shape
    alpha = bin_score.reshape(1, 1, 1).to(scores)
    C = torch.cat([torch.cat([scores, alpha.expand(b, m, 1)], 2), alpha.expand(b, 1, n + 1)], 1)
    norm = -torch.log(scores.new_tensor(float(m + n)))
    log_mu = torch.cat([norm.expand(m), (torch.log(scores.new_tensor(float(n))) + norm).reshape(1)])[None]
    log_nu = torch.cat([norm.expand(n), (torch.log(scores.new_tensor(float(m))) + norm).reshape(1)])[None]
    u, v = torch.zeros_like(log_mu).expand(b, -1), torch.zeros_like(log_nu).expand(b, -1)
    for _ in range(int(iters)):
        u = log_mu - torch.logsumexp(C + v[:, None, :], 2)
        v = log_nu - torch.logsumexp(C + u[:, :, None], 1)
    return C + u[:, :, None] + v[:, None, :] - norm


def mutual_matches(Z, threshold):
    """the extraction of superglue_train.py:276-286 on Z (B,m+1,n+1): (matches0 (B,m), matches1 (B,n), matching_scores0, matching_scores1);
    -1 where a keypoint has no mutual best partner above the threshold"""
    inner = Z[:, :-1, :-1]
    v0, i0 = inner.max(2)
    v1, i1 = inner.max(1)
    mutual0 = torch.arange(i0.shape[1], device=Z.device)[None] == i1.gather(1, i0)
    mutual1 = torch.arange(i1.shape[1], device=Z.device)[None] == i0.gather(1, i1)
    zero = Z.new_zeros(())
    ms0 = torch.where(mutual0, v0.exp(), zero)
    ms1 = torch.where(mutual1, ms0.gather(1, i1), zero)
    valid0 = mutual0 & (ms0 > threshold)
    valid1 = mutual1 & valid0.gather(1, i1)
    return torch.where(valid0, i0, i0.new_full((), -1)), torch.where(valid1, i1, i1.new_full((), -1)), ms0, ms1


class SuperGlueTrainable(nn.Module):
    """SuperGlueTrainable(config, engine): the reference's training SuperGlue with live parameters on engine's device.  `config` takes the
    reference's keys (DEFAULT_CONFIG; 'weights' is not read: load a checkpoint with load_state_dict).  engine = None builds the
    parameters only (state_dict, load_state_dict and the optimiser work; forward raises)."""
    default_config = DEFAULT_CONFIG

    def __init__(self, config, engine=None):
        super().__init__()
        self.config = {**self.default_config, **(config or {})}
        self.register_parameter('bin_score', nn.Parameter(torch.tensor(1.)))
        self.kenc, self.gnn, self.final_proj = build_modules(self.config)
        self.engine = engine
        if engine is not None:
            self.to(engine.device)

    def load_state_dict(self, state_dict, strict=True):
        """a checkpoint of the reference, as it stands or as the training script wraps it ({'net': state_dict, ...})"""
        if isinstance(state_dict, Mapping) and 'net' in state_dict and isinstance(state_dict['net'], Mapping):
            state_dict = state_dict['net']
        return super().load_state_dict(state_dict, strict)

    def _engine(self):
        if self.engine is None:
            raise ImxError("SuperGlueTrainable was built without an engine: there is no CPU path")
        return self.engine

    def _loss_and_scores(self, kpts0, scores0, desc0, kpts1, scores1, desc1, all_matches, n_all, shape0, shape1, n0, n1, matches=False, gt0=None):
        """(loss (B), scores); with matches=True (loss, scores, the dict of match_loss_matches) from the fused call -- the network part is
        the same code, so the loss and every gradient have the same bits either way"""
        eng = self._engine()
        dev = eng.device
        cnt = lambda c: None if c is None else torch.as_tensor(c).to(dev, torch.int32).contiguous()
        n0, n1 = cnt(n0), cnt(n1)
        f32 = lambda t: t.to(dev, torch.float32)
        # (desc may arrive as the transpose of Engine.train_pairs' (B,N,d): a sum keeps such strides, and the kernels take contiguous tensors)
        desc0 = f32(desc0).contiguous() + G.keypoint_encoder(eng, self.kenc, normalize_keypoints(f32(kpts0), shape0), f32(scores0).contiguous(), n=n0)
        desc1 = f32(desc1).contiguous() + G.keypoint_encoder(eng, self.kenc, normalize_keypoints(f32(kpts1), shape1), f32(scores1).contiguous(), n=n1)
        for layer, name in zip(self.gnn.layers, self.gnn.names):
            cross = name == 'cross'
            delta0 = G.gnn_layer(eng, layer, desc0, desc1 if cross else desc0, n=n0, ns=n1 if cross else n0)
            delta1 = G.gnn_layer(eng, layer, desc1, desc0 if cross else desc1, n=n1, ns=n0 if cross else n1)
            desc0, desc1 = desc0 + delta0, desc1 + delta1
        mdesc0 = G.conv1d(eng, desc0, self.final_proj.weight, self.final_proj.bias, n=n0)
        mdesc1 = G.conv1d(eng, desc1, self.final_proj.weight, self.final_proj.bias, n=n1)
        scores = G.scores(eng, mdesc0, mdesc1, n0, n1)
        if matches:
            loss, found = G.match_loss_matches(eng, scores, self.bin_score, all_matches, cnt(n_all), self.config['sinkhorn_iterations'],
                                               self.config['match_threshold'], n0, n1, gt0)
            return loss, scores, found
        return G.match_loss(eng, scores, self.bin_score, all_matches, cnt(n_all), self.config['sinkhorn_iterations'], n0, n1), scores

    def forward_pairs(self, kpts0, scores0, desc0, kpts1, scores1, desc1, all_matches, n_all, shape0, shape1, n0=None, n1=None):
        """The training forward on a padded batch of pairs -> the per-pair loss (B), differentiable with respect to every parameter.
        kpts (B,N,2) in pixels, scores (B,N), desc (B,d,N), all_matches (B,2,L) int64 and n_all (B) int32 as Engine.gt_matches returns
        them, shape0 / shape1 the image shapes (.., H, W), n0 / n1 (B) int32 counts or None = all.  Columns past a count are never read
        by a kernel and may hold anything.  BatchNorm follows the module's mode and updates its buffers in place in train mode."""
        return self._loss_and_scores(kpts0, scores0, desc0, kpts1, scores1, desc1, all_matches, n_all, shape0, shape1, n0, n1)[0]

    def forward_pairs_matches(self, kpts0, scores0, desc0, kpts1, scores1, desc1, all_matches, n_all, shape0, shape1, n0=None, n1=None, gt0=None):
        """forward_pairs with what the reference's forward reports beside the loss: (loss (B), {matches0 (B,N0), matches1 (B,N1) int64,
        matching_scores0, matching_scores1 fp32[, stats (B,3) int32 with gt0 (B,N0) int64]}), the matches extracted from the loss's own
        Sinkhorn (include/imx_sgloop.h).  The loss and its gradients have forward_pairs' bits; the dict's tensors require no grad.  Past
        the counts matches are -1 and scores 0."""
        loss, _, found = self._loss_and_scores(kpts0, scores0, desc0, kpts1, scores1, desc1, all_matches, n_all, shape0, shape1, n0, n1,
                                               matches=True, gt0=gt0)
        return loss, found

    def forward(self, data, want_matches=True):
        """The reference's forward on one sample of GlueSparse as the training loop hands it over: descriptors{0,1} (d,1,N), keypoints{0,1}
        (1,1,N,2), scores{0,1} (N,1), all_matches (2,1,L), image{0,1} (only .shape).  Returns 'loss' (shape (1,)) and 'skip_train': False;
        or the reference's early return with 'skip_train': True when a side has no keypoints.

        want_matches adds 'matches0/1' and 'matching_scores0/1', formed under torch.no_grad() by a PyTorch restatement of the optimal
        transport and the mutual-argmax extraction on the detached scores: that is a SECOND Sinkhorn, in PyTorch, beside the library's
        own inside the loss.  want_matches="loss" returns the same keys from the fused call instead (forward_pairs_matches): ONE Sinkhorn,
        the loss's, and the loss and every gradient keep the bits of want_matches=False.  A training loop passes "loss" or False."""
        desc0, desc1 = data['descriptors0'].transpose(0, 1).contiguous(), data['descriptors1'].transpose(0, 1).contiguous()
        kpts0, kpts1 = (torch.reshape(data[k], (1, data[k].numel() // 2, 2)) for k in ('keypoints0', 'keypoints1'))     # (an empty side too)
        if kpts0.shape[1] == 0 or kpts1.shape[1] == 0:                   # no keypoints (:238-246)
            shape0, shape1 = kpts0.shape[:-1], kpts1.shape[:-1]
            return {
                'matches0': kpts0.new_full(shape0, -1, dtype=torch.int)[0],
                'matches1': kpts1.new_full(shape1, -1, dtype=torch.int)[0],
                'matching_scores0': kpts0.new_zeros(shape0)[0],
                'matching_scores1': kpts1.new_zeros(shape1)[0],
                'skip_train': True
            }
        dev = self._engine().device
        all_matches = data['all_matches'].permute(1, 0, 2).to(dev, torch.int64).contiguous()      # (1, 2, L)
        n_all = torch.full((1,), all_matches.shape[2], dtype=torch.int32, device=dev)
        if isinstance(want_matches, str):
            if want_matches != "loss":
                raise ImxError(f"SuperGlueTrainable.forward: want_matches must be True, False or 'loss', got {want_matches!r}")
            loss, _, found = self._loss_and_scores(kpts0, torch.transpose(data['scores0'], 0, 1), desc0, kpts1, torch.transpose(data['scores1'], 0, 1),
                                                   desc1, all_matches, n_all, data['image0'].shape, data['image1'].shape, None, None, matches=True)
            return {'loss': loss, 'skip_train': False, **{k: v[0] for k, v in found.items()}}
        loss, scores = self._loss_and_scores(kpts0, torch.transpose(data['scores0'], 0, 1), desc0, kpts1, torch.transpose(data['scores1'], 0, 1),
                                             desc1, all_matches, n_all, data['image0'].shape, data['image1'].shape, None, None)
        out = {'loss': loss, 'skip_train': False}
        if want_matches:
            with torch.no_grad():
                Z = transport(scores.detach(), self.bin_score.detach(), self.config['sinkhorn_iterations'])
                m0, m1, ms0, ms1 = mutual_matches(Z, self.config['match_threshold'])
            out.update({'matches0': m0[0], 'matches1': m1[0], 'matching_scores0': ms0[0], 'matching_scores1': ms1[0]})
        return out
