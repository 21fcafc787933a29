"""The training loop of the reference's superpoint_glue_train.py:101-168 on the GPU: SuperGlueTrainer iterates epochs over a GlueSparse
dataset in batches, writes the reference's checkpoints, resumes, logs and draws the periodic match picture.

A step: dataset.batch(indices) (warp, SuperPoint on both images, the ground-truth assignment, all in libimx), the training forward of
sgtrain_model.SuperGlueTrainable.forward_pairs_matches (every layer in the libraries; the matches come from the loss's own Sinkhorn,
include/imx_sgloop.h), backward(), the optimiser: optim.FlatAdam (one launch, which zeroes the gradients too) or torch.optim.Adam as
the reference uses it (zero_grad(); backward(); step()).  Nothing inside a step waits for the device: the losses, the counts behind
precision and recall and the epoch's sum are accumulated on the device and read back every `log_interval` steps (the reference's 5) and
at the end of an epoch, one stacked copy each.

The loss of a batch is, by definition here, sum_b w_b loss_b / max(1, sum_b w_b) with w_b = 1 where both sides of pair b have
keypoints, formed on the device.  The reference runs batch size 1 and `continue`s on a sample without keypoints; here such a pair has
loss 0 and zero gradients (imx_ot_match_loss_grad), and a batch of nothing but such pairs still takes an optimiser step with zero
gradients: skipping it would need a host read inside the step.

Validation (not in the reference, whose loop has none): with a `val_dataset`, validate() runs after the checkpoint of every
`val_interval`-th epoch.  It walks the validation set in index order under a fixed dataset seed -- every validation sees the same warps --
in .eval() mode and under torch.no_grad(): forward_pairs_matches for the loss and the counts behind precision and recall, then the
measure of the SuperPoint and SuperGlue papers for pairs related by a homography: Engine.estimate_homography on the predicted matches
(include/imx_homog.h) and Engine.homography_corner_error against the known warp.  Everything accumulates on the device; ONE read-back
per validation.  It changes no parameter, BatchNorm buffer, optimiser state, shuffle generator or seed of the training set.

ONE GPU."""
import os
from collections.abc import Mapping
from pathlib import Path

import numpy as np
import torch

from .. import hostops
from ..optim import FlatAdam
from ..sgtrain_model import SuperGlueTrainable


def batch_loss(loss, counts0, counts1):
    """sum_b w_b loss_b / max(1, sum_b w_b), w_b = 1 where counts0[b] > 0 and counts1[b] > 0 -> a 0-d tensor on loss's device; no host read"""
    w = ((counts0 > 0) & (counts1 > 0)).to(loss.dtype)
    return (w * loss).sum() / w.sum().clamp(min=1.0)


def epoch_order(n, generator, shuffle):
    """the order of one epoch's samples: a permutation drawn from `generator` (a CPU torch.Generator, whose state the checkpoints carry),
    or 0..n-1"""
    return torch.randperm(n, generator=generator).tolist() if shuffle else list(range(n))


def epochs_to_run(done, total):
    """the epoch numbers a run that has finished `done` epochs still has to do: the reference's range(start_epoch + 1, opt.epoch + 1)"""
    return range(int(done) + 1, int(total) + 1)


def global_step(epoch, i, batches_per_epoch):
    """the step a scalar is logged under: len(train_loader) * (epoch - 1) + i + 1 (superpoint_glue_train.py:134)"""
    return batches_per_epoch * (epoch - 1) + i + 1


def _jet(values):
    try:
        import matplotlib.cm as cm
        return cm.jet(values)
    except ImportError:                     # a plain blue-to-red ramp
        v = np.clip(np.asarray(values, np.float64), 0, 1)
        return np.stack([v, np.zeros_like(v), 1 - v, np.ones_like(v)], -1)


class SuperGlueTrainer:
    """SuperGlueTrainer(config, dataset, engine, optimizer="flat" | "torch", lr=1e-4, ..., val_dataset=None, val_interval=1,
    val_batch_size=None (= batch_size), val_thresh=3.0 (pixels, the RANSAC threshold of the validation's fit)).  `config` is the SuperGlue config of the
    reference's script (descriptor_dim, keypoint_encoder, sinkhorn_iterations, match_threshold[, GNN_layers]); `dataset` has
    batch(indices) and __len__ (datasets.GlueSparse); engine = None builds the parameters and the optimiser state only (save, resume and
    the state dicts work; a step raises)."""

    def __init__(self, config, dataset, engine, optimizer="flat", lr=1e-4, batch_size=1, shuffle=True, seed=0, result_dir=None, writer=None,
                 log_interval=5, show_keypoints=True, viz_extension="png", max_steps=0, keep_losses=False, val_dataset=None, val_interval=1,
                 val_batch_size=None, val_thresh=3.0):
        if optimizer not in ("flat", "torch"):
            raise ValueError(f"SuperGlueTrainer: optimizer must be 'flat' or 'torch', got {optimizer!r}")
        if int(val_interval) < 1:
            raise ValueError(f"SuperGlueTrainer: val_interval must be at least 1 epoch, got {val_interval!r}")
        if val_batch_size is not None and int(val_batch_size) < 1:
            raise ValueError(f"SuperGlueTrainer: val_batch_size must be positive, got {val_batch_size!r}")
        if not float(val_thresh) > 0.0 or float(val_thresh) == float("inf"):
            raise ValueError(f"SuperGlueTrainer: val_thresh must be a positive number of pixels, got {val_thresh!r}")
        self.config, self.dataset, self.engine = dict(config or {}), dataset, engine
        self.net = SuperGlueTrainable(self.config, engine).train()
        self.optimizer_kind, self.lr = optimizer, float(lr)
        if optimizer == "flat":
            self.optimizer = FlatAdam(self.net.parameters(), engine, lr=self.lr)
        else:
            self.optimizer = torch.optim.Adam(self.net.parameters(), lr=self.lr)
        self.batch_size, self.shuffle, self.seed = int(batch_size), bool(shuffle), int(seed)
        self.generator = torch.Generator().manual_seed(self.seed)
        self.result_dir = None if result_dir is None else str(result_dir)
        self.writer, self.log_interval = writer, int(log_interval)
        self.show_keypoints, self.viz_extension = bool(show_keypoints), viz_extension
        self.max_steps, self.keep_losses = int(max_steps), bool(keep_losses)
        self.epoch = 0                      # epochs finished
        self.steps = 0                      # optimiser steps taken by this object
        self.step_losses = []               # with keep_losses: every step's batch loss, a 0-d device tensor (never read here)
        self.history = []                   # (tag, step, value) of every scalar read back
        self.last = None                    # the last step's batch and matches, for the picture
        self._data_seed = None
        self.val_dataset, self.val_interval, self.val_thresh = val_dataset, int(val_interval), float(val_thresh)
        self.val_batch_size = self.batch_size if val_batch_size is None else int(val_batch_size)
        self._val_seed = int(getattr(val_dataset, "seed", 0)) if val_dataset is not None else None      # the warps of EVERY validation
        self.last_validation = None         # the scalars of the last validate(), a dict
        self._reset_accumulators()

    # ---------------------------------------------------------------------------------------------- one step
    def _device(self):
        return self.net.bin_score.device

    def _reset_accumulators(self):
        dev = self._device()
        self._loss_sum = torch.zeros((), dtype=torch.float32, device=dev)
        self._loss_n = 0
        self._epoch_sum = torch.zeros((), dtype=torch.float32, device=dev)
        self._stats_sum = torch.zeros(3, dtype=torch.int64, device=dev)

    def _optimise(self, loss):
        if self.optimizer_kind == "flat":
            loss.backward()
            self.optimizer.step()           # one launch; it leaves the gradients zero, which is the zero_grad() of the next step
        else:
            self.optimizer.zero_grad()
            loss.backward()
            self.optimizer.step()

    def train_step(self, batch):
        """One optimiser step on dataset.batch(indices) for a list of indices, or on one sample dict of the reference's loop (a batch-1
        DataLoader's: descriptors (d,1,N), keypoints (1,1,N,2), scores (N,1), all_matches (2,1,L), image0/1).  Returns the batch loss, a
        0-d device tensor; nothing is read back."""
        with torch.enable_grad():
            if isinstance(batch, Mapping):
                out = self.net(batch, want_matches="loss")
                if out["skip_train"]:       # a side without keypoints: the step is taken with zero gradients (see the module docstring)
                    loss = sum((p * 0).sum() for p in self.net.parameters())
                else:
                    loss = out["loss"].reshape(())
                found, b = {k: v[None] for k, v in out.items() if k not in ("loss", "skip_train")}, None
            else:
                b = self.dataset.batch(list(batch))
                shape = tuple(b["image0"].shape[-2:])
                per_pair, found = self.net.forward_pairs_matches(
                    b["keypoints0"], b["scores0"], b["descriptors0"].transpose(1, 2), b["keypoints1"], b["scores1"], b["descriptors1"].transpose(1, 2),
                    b["all_matches"], b["n_all"], shape, shape, n0=b["counts0"], n1=b["counts1"], gt0=b["gt0"])
                loss = batch_loss(per_pair, b["counts0"], b["counts1"])
            self._optimise(loss)
        value = loss.detach()
        self._loss_sum = self._loss_sum + value
        self._epoch_sum = self._epoch_sum + value
        self._loss_n += 1
        if "stats" in found:
            self._stats_sum = self._stats_sum + found["stats"].sum(0)
        if self.keep_losses:
            self.step_losses.append(value)
        self.steps += 1
        self.last = (b, found)
        return value

    # ---------------------------------------------------------------------------------------------- logging
    def _scalar(self, tag, value, step):
        self.history.append((tag, int(step), float(value)))
        if self.writer is not None:
            self.writer.add_scalar(tag, float(value), int(step))

    def log(self, epoch, epochs, i, batches):
        """the reference's every-5-steps block (:132-157): the mean loss since the last one, precision and recall of matches0 against the
        ground truth over the same steps -- ONE read-back -- and the match picture of the last step's first pair"""
        row = torch.cat([(self._loss_sum / max(self._loss_n, 1)).reshape(1).double(), self._stats_sum.double()]).cpu().tolist()
        mean_loss, (n_gt, n_pred, n_ok) = row[0], (int(v) for v in row[1:])
        step = global_step(epoch, i, batches)
        self._scalar("Mean_Loss", mean_loss, step)
        self._scalar("precision", n_ok / max(n_pred, 1), step)
        self._scalar("recall", n_ok / max(n_gt, 1), step)
        print('Epoch [{}/{}], Step [{}/{}], Mean Loss: {:.4f}'.format(epoch, epochs, i + 1, batches, mean_loss))
        self._loss_sum, self._loss_n = torch.zeros_like(self._loss_sum), 0
        self._stats_sum = torch.zeros_like(self._stats_sum)
        if self.result_dir is not None and self.last is not None and self.last[0] is not None:
            self.draw(Path(self.result_dir, "match", "{}_matches.{}".format(i, self.viz_extension)))

    def draw(self, path):
        """the match picture of the last step's first pair (:141-157), through hostops.make_matching_plot_fast.  The matches are the
        training forward's own: the reference switches to .eval() here without running a forward, which changes nothing it draws."""
        b, found = self.last
        n0, n1 = int(b["counts0"][0]), int(b["counts1"][0])
        kpts0, kpts1 = b["keypoints0"][0, :n0].cpu().numpy(), b["keypoints1"][0, :n1].cpu().numpy()
        matches, conf = found["matches0"][0, :n0].cpu().numpy(), found["matching_scores0"][0, :n0].cpu().numpy()
        valid = matches > -1
        os.makedirs(os.path.dirname(str(path)), exist_ok=True)
        stem = os.path.basename(str(b["file_name"][0]))
        hostops.make_matching_plot_fast(b["image0"][0].cpu().numpy(), b["warped"][0].cpu().numpy(), kpts0, kpts1, kpts0[valid], kpts1[matches[valid]],
                                        _jet(conf[valid]), [], path=path, show_keypoints=self.show_keypoints,
                                        small_text=["Matches: {}".format(int(valid.sum())), stem])
        return str(path)

    # ---------------------------------------------------------------------------------------------- validation
    def _val_batches(self):
        """the index lists of one validation pass: index order, every sample (no drop_last)"""
        n = len(self.val_dataset)
        return [list(range(i, min(i + self.val_batch_size, n))) for i in range(0, n, self.val_batch_size)]

    def _validate_batch(self, b):
        """one validation batch, under the caller's mode and grad setting: (per-pair loss (B), the dict of forward_pairs_matches, the
        corner error (B) float64 of the homography fitted to matches0 against b['M']); nothing is read back"""
        shape = tuple(b["image0"].shape[-2:])
        per_pair, found = self.net.forward_pairs_matches(
            b["keypoints0"], b["scores0"], b["descriptors0"].transpose(1, 2), b["keypoints1"], b["scores1"], b["descriptors1"].transpose(1, 2),
            b["all_matches"], b["n_all"], shape, shape, n0=b["counts0"], n1=b["counts1"], gt0=b["gt0"])
        H, _, _, _ = self.engine.estimate_homography(b["keypoints0"].float().contiguous(), b["keypoints1"].float().contiguous(), found["matches0"],
                                                     counts0=b["counts0"], ransac_thresh=self.val_thresh)
        return per_pair, found, self.engine.homography_corner_error(H, b["M"], shape)

    def validate(self, epoch):
        """One pass over val_dataset (see the module docstring) -> dict of the scalars, also written through _scalar under `epoch` and
        printed on one line: val_loss (sum_b w_b loss_b / max(1, sum_b w_b) over ALL pairs, w_b as in batch_loss), val_precision,
        val_recall, val_corner_error_median (of the mean corner error per pair, in pixels; a failed fit is +inf and stays in the order
        statistics: the median of an even count is the mean of the two middle ones), val_homography_correct_1 / _3 / _5 (the share of
        pairs whose corner error is below that many pixels).  The net is left in the mode it was in."""
        if self.val_dataset is None:
            raise RuntimeError("SuperGlueTrainer.validate: no val_dataset")
        if len(self.val_dataset) == 0:
            raise RuntimeError("SuperGlueTrainer.validate: the validation set is empty")
        ds, was_training = self.val_dataset, self.net.training
        had_seed, old_seed = hasattr(ds, "seed"), getattr(ds, "seed", None)
        dev = self._device()
        loss_sum, w_sum = torch.zeros((), dtype=torch.float32, device=dev), torch.zeros((), dtype=torch.float32, device=dev)
        stats, errors = torch.zeros(3, dtype=torch.int64, device=dev), []
        self.net.eval()
        try:
            if had_seed:
                ds.seed = self._val_seed
            with torch.no_grad():
                for indices in self._val_batches():
                    b = ds.batch(indices)
                    per_pair, found, err = self._validate_batch(b)
                    w = ((b["counts0"] > 0) & (b["counts1"] > 0)).to(per_pair.dtype)
                    loss_sum, w_sum = loss_sum + (w * per_pair).sum(), w_sum + w.sum()
                    stats = stats + found["stats"].sum(0)
                    errors.append(err)
                err = torch.sort(torch.cat(errors))[0]
                n = err.numel()
                lo, hi = err[(n - 1) // 2], err[n // 2]
                median = torch.where(lo == hi, lo, 0.5 * (lo + hi))          # (inf + inf stays inf; no inf - inf anywhere)
                row = torch.cat([(loss_sum / w_sum.clamp(min=1.0)).reshape(1).double(), stats.double(), median.reshape(1),
                                 torch.stack([(err < k).double().mean() for k in (1.0, 3.0, 5.0)])]).cpu().tolist()      # the ONE read-back
        finally:
            if had_seed:
                ds.seed = old_seed
            self.net.train(was_training)
        n_gt, n_pred, n_ok = (int(v) for v in row[1:4])
        out = {"val_loss": row[0], "val_precision": n_ok / max(n_pred, 1), "val_recall": n_ok / max(n_gt, 1), "val_corner_error_median": row[4],
               "val_homography_correct_1": row[5], "val_homography_correct_3": row[6], "val_homography_correct_5": row[7]}
        for tag, value in out.items():
            self._scalar(tag, value, epoch)
        print("Validation [{}]: ".format(epoch) + ", ".join("{} {:.4f}".format(k, v) for k, v in out.items()))
        self.last_validation = out
        return out

    # ---------------------------------------------------------------------------------------------- the loop
    def train(self, epochs):
        """superpoint_glue_train.py:101-168 from the epoch after the last finished one to `epochs`: an optional seeded shuffle, batches of
        batch_size with drop_last, 'Mean_Loss' every log_interval steps, 'epoch_loss' and a checkpoint at the end of every epoch.  The
        dataset's warps of an epoch follow from (its seed, the epoch): every epoch sees new warps, a resumed run the ones the
        uninterrupted run saw.  max_steps > 0 ends the run after that many steps, with a checkpoint of the epoch it stands in.  With a
        validation set, validate(epoch) follows the checkpoint of every val_interval-th epoch."""
        n = len(self.dataset)
        batches = n // self.batch_size
        if batches == 0:
            raise RuntimeError(f"SuperGlueTrainer.train: {n} samples make no batch of {self.batch_size} (drop_last)")
        taken = 0
        for epoch in epochs_to_run(self.epoch, epochs):
            if hasattr(self.dataset, "seed"):
                if self._data_seed is None:
                    self._data_seed = int(self.dataset.seed)
                self.dataset.seed = self._data_seed + epoch - 1
            order = epoch_order(n, self.generator, self.shuffle)
            self._reset_accumulators()
            cut = False
            for i in range(batches):
                self.train_step(order[i * self.batch_size:(i + 1) * self.batch_size])
                taken += 1
                if (i + 1) % self.log_interval == 0:
                    self.log(epoch, epochs, i, batches)
                if self.max_steps and taken >= self.max_steps:
                    cut = True
                    break
            epoch_loss = float(self._epoch_sum.item()) / batches
            self._scalar("epoch_loss", epoch_loss, epoch)
            self.epoch = epoch
            where = self.save(epoch)
            print("Epoch [{}/{}] done. Epoch Loss {}. Checkpoint saved to {}".format(epoch, epochs, epoch_loss, where))
            if self.val_dataset is not None and epoch % self.val_interval == 0:
                self.validate(epoch)
            if cut:
                break
        return self.epoch

    # ---------------------------------------------------------------------------------------------- checkpoints
    def checkpoint(self, epoch):
        """{'epoch', 'net'} exactly as the reference writes them (:166), then 'optimizer' (torch.optim.Adam's state-dict format, from
        either optimiser) and 'rng' (the shuffle generator's state); the reference's loader reads the first two only"""
        return {"epoch": int(epoch), "net": type(self.net.state_dict())((k, v.detach().clone()) for k, v in self.net.state_dict().items()),
                "optimizer": self.optimizer.state_dict(), "rng": self.generator.get_state()}

    def save(self, epoch):
        """<result_dir>/checkpoints/SuperGlue_epoch_{epoch}.pth -> its directory (what the reference prints)"""
        if self.result_dir is None:
            raise RuntimeError("SuperGlueTrainer.save: no result_dir")
        out = self.result_dir + "/checkpoints"
        os.makedirs(out, exist_ok=True)
        torch.save(self.checkpoint(epoch), out + "/SuperGlue_epoch_{}.pth".format(epoch))
        return out

    def load_checkpoint(self, checkpoint):
        """a checkpoint of save(), or one of the reference's with 'epoch' and 'net' only: the optimiser then starts fresh, as the
        reference's does, and the shuffle's generator stays where it is"""
        self.net.load_state_dict(checkpoint["net"])
        self.epoch = int(checkpoint["epoch"])
        if "optimizer" in checkpoint:
            self.optimizer.load_state_dict(checkpoint["optimizer"])
        if "rng" in checkpoint:
            self.generator.set_state(checkpoint["rng"].cpu())
        return self.epoch

    def resume(self, path):
        return self.load_checkpoint(torch.load(str(path), map_location=self._device()))
