"""Writes the fixtures of the trainable SuperPoint network from the REFERENCE's own inconv and down blocks under torch.autograd (imported
unchanged; never runs where the reference is absent):

    python tests/golden/make_golden_sppool.py --reference /path/to/reference

The reference's SuperPoint class cannot be imported (its utils need cv2), so the network is tests/sppool_ref.py: Net built from the
reference's unet_parts.inconv and unet_parts.down, the heads torch's own modules arranged as superpoint_train.py:20-28 and 47-54 arrange
them.  Two cases at descriptor_length = 128 (tests/sppool_ref.py: NET_CASES): `even` (2,1,16,24) and `odd` (2,1,18,27), where floor
pooling drops a row or a column at every level.  Inputs and parameters are NOT stored: the tests re-derive them from the seed
(conv3grad_ref.block_state's recipe over the whole network, sppool_ref.net_case).  spmodel_<case>.npz holds, from one training step in
fp32 and float64 on the CPU:

  seed, refused, refused_why      the seed taken, the seeds refused before it, and per refused seed the three counts of sppool_ref.unsafe
  names                           semi, desc, dx and the 48 parameters
  <i>_g, <i>_d32, <i>_sum         per tensor i of names: the float64 value at sppool_ref.net_positions(i) (up to 400), the fp32 run's value
                                  minus it, and the float64 sum of the whole tensor
  buffer_names, buffer_<i>        every buffer of the float64 module after the step
  eval_semi_g/_d32, eval_desc_g/_d32   the outputs in .eval() mode from the same seeded state, at net_positions(0) and (1)
  adam_g, adam_d32                `even` only: the float64 losses of 4 Adam steps (lr 1e-3) on mean((semi - t_s)^2) + mean((desc - t_d)^2)
                                  and the fp32 run's minus them

The seed rule: from the starting seed upward the first seed is taken at which, in float64, no BatchNorm output that a ReLU follows lies
within 1e-5 of 0, no pooling window has its two largest values positive and closer than 1e-5 (there the routing of the gradient jumps),
no descriptor vector is zero, and every result is finite.  At most MAX_TRIES seeds are tried; beyond that the generator fails."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import sppool_ref as RP   # noqa: E402

MAX_TRIES = 400
SEED0 = {"even": 101, "odd": 601}


def make(parts, seed, dtype, train=True):
    m = RP.load_net(RP.Net(RP.D_NET, parts.inconv, parts.down), seed, dtype)
    return m.train(train)


def run(parts, name, seed, dtype):
    x, dy_s, dy_d, t_s, t_d = (torch.from_numpy(a).to(dtype) for a in RP.net_case(seed, name))
    m = make(parts, seed, dtype)
    res = {k: v.double().numpy() for k, v in RP.net_grads(m, x, dy_s, dy_d).items()}
    buffers = RP.net_buffers(m)
    with torch.no_grad():
        ev = make(parts, seed, dtype, train=False)(x.clone())
    ev = {k: v.double().numpy() for k, v in ev.items()}
    losses = np.array(RP.adam_losses(make(parts, seed, dtype), x, t_s, t_d), np.float64) if name == "even" else None
    return res, buffers, ev, losses


def build(parts, name):
    refused, why = [], []
    for seed in range(SEED0[name], SEED0[name] + MAX_TRIES):
        x64 = torch.from_numpy(RP.net_case(seed, name)[0]).double()
        counts = RP.unsafe(make(parts, seed, torch.float64), x64)
        if any(counts):
            refused.append(seed)
            why.append(counts)
            continue
        r64, buffers, e64, l64 = run(parts, name, seed, torch.float64)
        r32, _, e32, l32 = run(parts, name, seed, torch.float32)
        if not all(np.isfinite(a).all() for a in list(r64.values()) + list(r32.values()) + list(e64.values()) + list(e32.values())):
            refused.append(seed)
            why.append((-1, -1, -1))
            continue
        assert len(r64) == 3 + 48
        fx = {"seed": np.int64(seed), "refused": np.array(refused, np.int64), "refused_why": np.array(why, np.int64).reshape(-1, 3),
              "names": np.array(list(r64))}
        for i, (key, a) in enumerate(r64.items()):
            pos = RP.net_positions(i, a.size)
            fx.update({f"{i}_g": a.reshape(-1)[pos], f"{i}_d32": (r32[key] - a).reshape(-1)[pos].astype(np.float32),
                       f"{i}_sum": a.sum(keepdims=True).reshape(1)})
        fx["buffer_names"] = np.array(list(buffers))
        fx.update({f"buffer_{i}": b for i, b in enumerate(buffers.values())})
        for i, key in enumerate(("semi", "desc")):
            pos = RP.net_positions(i, e64[key].size)
            fx.update({f"eval_{key}_g": e64[key].reshape(-1)[pos], f"eval_{key}_d32": (e32[key] - e64[key]).reshape(-1)[pos].astype(np.float32)})
        if l64 is not None:
            fx.update({"adam_g": l64, "adam_d32": (l32 - l64).astype(np.float32)})
        return fx
    return f"no seed from {SEED0[name]} passed in {MAX_TRIES} tries"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.reference, "superpoint", "models"))
    import unet_parts                                   # noqa: E402  (the reference's, unchanged)
    failed = []
    for name in RP.NET_CASES:
        fx = build(unet_parts, name)
        if isinstance(fx, str):
            print(f"spmodel_{name}.npz REFUSED: {fx}")
            failed.append(name)
            continue
        path = os.path.join(HERE, f"spmodel_{name}.npz")
        np.savez_compressed(path, **fx)
        size = os.path.getsize(path)
        assert size < 400000, f"{path}: {size} bytes"
        print(f"spmodel_{name}.npz: {size} bytes, {len(fx)} arrays, seed {int(fx['seed'])}, refused {len(fx['refused'])} seeds")
    assert not failed, f"committed cases were refused: {failed}"


if __name__ == "__main__":
    main()
