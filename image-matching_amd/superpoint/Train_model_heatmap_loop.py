"""The training loop of the reference's descriptor-training agent (superpoint/Train_model_heatmap.py:33-430 on
Train_model_frontend.py:88-353) on the GPU: `Train_model_heatmap` here is a subclass of the forward-only agent of
superpoint/Train_model_heatmap.py (which stays as it is and whose train() still raises) with loadModel, train_val_sample(train=True),
train() and saveModel().  It is the import swap for superpoint_train_descriptor.py:10.

A step: both forwards of SuperPointTrainable (every layer in the libraries), sptrain_grad.total_loss (both detector losses and the
sparse descriptor loss, value and gradient in the library) on the `*_gaussian` label maps when data.gaussian_label is enabled
(Train_model_heatmap.py:135-142), backward(), FlatAdam.step() (one launch, which zeroes the gradients too).  Nothing inside a step
waits for the device; scalars are read back every tensorboard_interval steps and on validation only.

With the top-level config key `validation_metrics: {enable: true, pairs: 16, max_keypoints: 1000, eps: 3, keep_best: true}` train() also
calls validate_metrics() at every validation_interval, after the checkpoint of that iteration and after the loss validation: what the
DEPLOYED network would do from the present weights (superpoint/validation.py: repeatability, localisation error, matching score,
homography correctness), as one ("metrics", n_iter, {...}) row of `history`, and with keep_best a superPointNet_best_checkpoint.pth.tar
whenever val_homography_correct_3 improves (ties: val_repeatability).  It acts on a copy of the state dict and leaves the network, the
optimiser, the loaders' datasets' seeds and every generator as they were.  Absent or off: nothing changes.

ONE GPU: dataParallel() keeps the single-device model and says so.  Not served, raising as in the base class: detector_loss 'l2',
dense_loss; add_res_loss / pred_soft_argmax and a subpixel head raise here; images and histograms are not written to the writer."""
import copy
import logging
import os
from pathlib import Path

import torch
import torch.nn.functional as F

from .. import sptrain, sptrain_grad
from ..datasets.ALLSS_train import check_gaussian_label
from ..optim import FlatAdam
from ..sptrain_model import SuperPointTrainable
from .Train_model_heatmap import Train_model_heatmap as _ForwardOnly

SCALAR_KEYS = ("loss", "loss_det", "loss_det_warp", "positive_dist", "negative_dist")
METRICS_DEFAULT = {"enable": False, "pairs": 16, "max_keypoints": 1000, "eps": 3, "keep_best": True}
BEST_NAME = "superPointNet_best_checkpoint.pth.tar"


class BatchLoader:
    """The loop's `train_loader` / `val_loader`: a dataset with batch(indices) plus a batch size.  Iterating yields device batches in
    index order (the reference's DataLoader(shuffle=False)); the last batch may be smaller."""

    def __init__(self, dataset, batch_size):
        self.dataset, self.batch_size = dataset, int(batch_size)

    def __len__(self):
        return -(-len(self.dataset) // self.batch_size)

    def __iter__(self):
        return self.from_batch(0)

    def from_batch(self, first):
        """the batches of one epoch from batch `first` on (a resumed run enters its first epoch where the interrupted one stood)"""
        n = len(self.dataset)
        for i0 in range(first * self.batch_size, n, self.batch_size):
            yield self.dataset.batch(range(i0, min(i0 + self.batch_size, n)))


class _Recorder:
    """Hands sptrain_grad.total_loss the engine's two value-and-gradient calls and keeps what they returned beside the gradients: the
    detector losses and the descriptor loss's mean row, which the scalar dictionary needs"""

    def __init__(self, engine):
        self.engine, self.det, self.desc = engine, [], None

    def detector_loss_grad(self, *a, **k):
        out, grad = self.engine.detector_loss_grad(*a, **k)
        self.det.append(out)
        return out, grad

    def desc_loss_sparse_grad(self, *a, **k):
        res = self.engine.desc_loss_sparse_grad(*a, **k)
        self.desc = res["mean"]
        return res


class Train_model_heatmap(_ForwardOnly):
    default_config = dict(_ForwardOnly.default_config, validation_interval=2000, validation_size=5, retrain=True, reset_iter=True,
                          pretrained=None, seed=0)

    def __init__(self, config, save_path=Path("."), device="cuda", verbose=False):
        g = (config.get("data") or {}).get("gaussian_label") or {}
        self.gaussian = bool(g.get("enable", False))
        base = config
        if self.gaussian:
            check_gaussian_label(g)
            base = copy.deepcopy(config)
            base["data"]["gaussian_label"]["enable"] = False          # the forward-only agent raises on the flag
        super().__init__(base, save_path=save_path, device=device, verbose=verbose)
        self.config = config
        model = config["model"]
        if model.get("add_res_loss") or model.get("pred_soft_argmax") or (model.get("subpixel") or {}).get("enable"):
            raise NotImplementedError("add_res_loss / pred_soft_argmax / subpixel are not served: only the shipped yaml's objective")
        self.max_iter = int(config.get("train_iter", self.default_config["train_iter"]))
        self.seed = int(config.get("seed", 0))
        self.n_iter = 0
        self.loss = None
        self.optimizer = None
        self.engine = None
        self.writer = None
        self.train_loader = self.val_loader = None
        self._data_seed = None
        self.history = []                 # (task, n_iter, {scalar: float}) of every read-back
        self.metrics_config = dict(METRICS_DEFAULT, **(config.get("validation_metrics") or {}))
        self.validator = None             # superpoint/validation.py's, made at the first validate_metrics()
        self.best = None                  # (val_homography_correct_3, val_repeatability) of the best checkpoint written so far

    # ---------------------------------------------------------------------------------------------- model and optimiser
    def loadModel(self, state_dict=None):
        """Train_model_frontend.py:307-338: the trainable network and Adam(lr=model.learning_rate, betas=(0.9, 0.999)); with
        retrain false, `pretrained` is loaded: a '.pth' file is a bare model state dict, anything else a full checkpoint (model,
        optimiser, n_iter); reset_iter puts the iteration count back to 0.  Training resumes at the number of steps the checkpoint had taken."""
        model = self.config["model"]
        d = int(model.get("descriptor_length", 256))
        self.engine = sptrain.plain_engine(self.device, d)
        self.net = SuperPointTrainable(self.engine, d).train()
        if state_dict is not None:
            self.net.load_state_dict(state_dict)
        self.optimizer = FlatAdam(self.net.parameters(), self.engine, lr=float(model.get("learning_rate", 1e-4)), betas=(0.9, 0.999))
        n_iter = 0
        if not self.config.get("retrain", True):
            path = str(self.config["pretrained"])
            logging.info("load pretrained model from: %s", path)
            checkpoint = torch.load(path, map_location=self.engine.device)
            if path[-4:] == ".pth":
                self.net.load_state_dict(checkpoint)
            else:
                self.net.load_state_dict(checkpoint["model_state_dict"])
                self.optimizer.load_state_dict(checkpoint["optimizer_state_dict"])
                # saveModel stores n_iter + 1, as the reference does; the steps taken are one fewer.  (The reference's loader takes the
                # stored value as it is and so skips one iteration number at every resume.  Here a resumed run must repeat the
                # uninterrupted one bit for bit, and the draws and the loader's position are keyed by the iteration.)
                n_iter = max(int(checkpoint["n_iter"]) - 1, 0)
        if self.config.get("reset_iter", True):
            logging.info("reset iterations to 0")
            n_iter = 0
        self.n_iter = n_iter
        return self.net

    def dataParallel(self):
        logging.info("=== one GPU: image_matching_amd's training loop has no data parallelism (the reference wraps the net in nn.DataParallel here)")
        return self.net

    # ---------------------------------------------------------------------------------------------- one step
    def _generator(self, n_iter):
        """the descriptor-loss draws of iteration n_iter: a device generator seeded by (seed, n_iter), so a resumed run draws what the
        uninterrupted one drew"""
        g = torch.Generator(device=self.engine.device)
        g.manual_seed((self.seed * 1000003 + int(n_iter)) % (1 << 63))
        return g

    def train_val_sample(self, sample, n_iter=0, train=False):
        """Train_model_heatmap.py:83-314 on a batch of ALLSSTrain.batch(indices): returns the scalar dictionary (:246-254) as 0-d device
        tensors -- loss, loss_det, loss_det_warp, positive_dist, negative_dist, and, every tensorboard_interval iterations and on
        validation, precision and recall of the heatmap of the network being trained."""
        if self.net is None:
            self.loadModel()
        if "warped_img" not in sample:
            raise NotImplementedError("the training objective needs data.warped_pair.enable (the shipped yaml)")
        task = "train" if train else "val"
        eng, p, model = self.engine, self.desc_params, self.config["model"]
        img, img_warp = sample["image"], sample["warped_img"]
        B, H, W = img.shape[0], img.shape[-2], img.shape[-1]
        # (the net stays in train mode on validation batches too, as the reference's does: batch statistics, and the running ones move)
        with torch.set_grad_enabled(train):
            outs = self.net(img.contiguous())
            semi, desc = outs["semi"], outs["desc"]
            outs_warp = self.net(img_warp.contiguous())
            semi_warp, desc_warp = outs_warp["semi"], outs_warp["desc"]
            choice, non = sptrain.draw(eng, sample["homographies"], H // 8, W // 8, int(p.get("num_matching_attempts", 1000)),
                                       int(p.get("num_masked_non_matches_per_match", 10)), self._generator(n_iter))
            s = dict(sample, choice=choice, nonmatch_b=non)
            if self.gaussian:             # Train_model_heatmap.py:135-142
                s["labels_2D"], s["warped_labels"] = sample["labels_2D_gaussian"], sample["warped_labels_gaussian"]
            rec = _Recorder(eng)
            loss = sptrain_grad.total_loss(rec, semi, semi_warp, desc, desc_warp, s, lambda_loss=model.get("lambda_loss", 1),
                                           lamda_d=p.get("lamda_d", 250), method=p.get("method", "1d"))
        self.loss = loss.detach()
        self.scalar_dict = {"loss": self.loss, "loss_det": rec.det[0][0], "loss_det_warp": rec.det[1][0], "positive_dist": rec.desc[1],
                            "negative_dist": rec.desc[2]}
        if train:
            loss.backward()
            self.optimizer.step()         # one launch; it leaves the gradients zero, which is the reference's zero_grad() of the next step
        tb_interval = int(self.config.get("tensorboard_interval", 200))
        if n_iter % tb_interval == 0 or task == "val":
            with torch.no_grad():         # add2tensorboard_nms (:287-309): flattenDetection, then heatmap_to_nms against labels_2D
                dense = F.softmax(semi.detach(), dim=1)[:, :-1]
                heatmap = F.pixel_shuffle(dense, 8)
                pred = self.heatmap_to_nms(eng, heatmap)
                self.scalar_dict.update(self.batch_precision_recall(pred, sample["labels_2D"]))
            self._report(task, n_iter)
        self.outputs = {"semi": semi.detach(), "semi_warp": semi_warp.detach(), "desc": desc.detach(), "desc_warp": desc_warp.detach()}
        return self.scalar_dict

    def _report(self, task, n_iter):
        """the one place a step's scalars are read back: one stacked copy"""
        keys = list(self.scalar_dict)
        values = torch.stack([self.scalar_dict[k].reshape(()).float() for k in keys]).cpu().tolist()
        row = dict(zip(keys, values))
        self.history.append((task, int(n_iter), row))
        logging.info("%s iter %d: %s", task, n_iter, ", ".join(f"{k}: {v:.4f}" for k, v in row.items()))
        if self.writer is not None:
            for k, v in row.items():
                self.writer.add_scalar(task + "-" + k, v, n_iter)

    # ---------------------------------------------------------------------------------------------- the loop
    def train(self, **options):
        """Train_model_frontend.py:88-117"""
        if self.net is None:
            self.loadModel()
        if self.train_loader is None:
            raise RuntimeError("train(): set train_loader (and val_loader) first: BatchLoader(dataset, batch_size)")
        logging.info("n_iter: %d", self.n_iter)
        logging.info("max_iter: %d", self.max_iter)
        epoch = 0
        while self.n_iter < self.max_iter:
            logging.info("epoch: %d", epoch)
            epoch += 1
            steps = 0
            # every epoch draws its own homographies and augmentations: the dataset's draws are keyed by (seed, index), and the seed of
            # an epoch follows from the iteration, like ...
            ds = getattr(self.train_loader, "dataset", None)
            if ds is not None and hasattr(ds, "seed") and hasattr(self.train_loader, "from_batch"):
                if self._data_seed is None:
                    self._data_seed = int(ds.seed)
                ds.seed = self._data_seed + self.n_iter // len(self.train_loader)
            # ... the position within the epoch, so a resumed run sees the batches the uninterrupted one saw
            batches = self.train_loader.from_batch(self.n_iter % len(self.train_loader)) if hasattr(self.train_loader, "from_batch") else self.train_loader
            for sample_train in batches:
                self.train_val_sample(sample_train, self.n_iter, True)
                self.n_iter += 1
                steps += 1
                if self.val_loader is not None and self.n_iter % int(self.config["validation_interval"]) == 0:
                    logging.info("====== Validating...")
                    for j, sample_val in enumerate(self.val_loader):
                        self.train_val_sample(sample_val, self.n_iter + j, False)
                        if j > int(self.config.get("validation_size", 3)):
                            break
                if self.n_iter % int(self.config["save_interval"]) == 0:
                    logging.info("save model: every %d interval, current iteration: %d", int(self.config["save_interval"]), self.n_iter)
                    self.saveModel()
                if self.metrics_config["enable"] and self.n_iter % int(self.config["validation_interval"]) == 0:
                    self.validate_metrics()
                if self.n_iter >= self.max_iter:       # (the reference tests > and so runs one step past train_iter; this loop stops at it)
                    logging.info("End training: %d", self.n_iter)
                    break
            if steps == 0:
                raise RuntimeError("train(): the train loader is empty")

    # ---------------------------------------------------------------------------------------------- the deployed network's metrics
    def validate_metrics(self):
        """One pass of superpoint/validation.py's SuperPointValidator over the first `pairs` samples of the validation set, on a COPY of
        the present state dict: the scalars to the writer, one ("metrics", n_iter, row) to history, and with keep_best the best
        checkpoint.  Returns the row."""
        from .validation import SuperPointValidator
        if self.net is None:
            self.loadModel()
        m = self.metrics_config
        if self.validator is None:
            loader = self.val_loader if self.val_loader is not None else self.train_loader
            if loader is None:
                raise RuntimeError("validate_metrics(): set val_loader (or train_loader) first")
            self.validator = SuperPointValidator(self.config, loader.dataset, self.device, max_keypoints=int(m["max_keypoints"]), eps=float(m["eps"]),
                                                 pairs=int(m["pairs"]), batch_size=getattr(loader, "batch_size", None), seed=self.seed)
            best_path = os.path.join(str(self.save_path), BEST_NAME)
            if m["keep_best"] and not self.config.get("retrain", True) and os.path.exists(best_path):      # a resumed run: the incumbent
                kept = torch.load(best_path, map_location="cpu").get("metrics") or {}
                if "val_homography_correct_3" in kept and "val_repeatability" in kept:
                    self.best = (float(kept["val_homography_correct_3"]), float(kept["val_repeatability"]))
        state = {k: v.detach().clone() for k, v in self.net.state_dict().items()}
        row = self.validator.evaluate(state)
        self.history.append(("metrics", int(self.n_iter), row))
        logging.info("metrics iter %d: %s", self.n_iter, ", ".join(f"{k}: {v:.4f}" for k, v in row.items()))
        if self.writer is not None:
            for k, v in row.items():
                self.writer.add_scalar(k, v, self.n_iter)
        key = (row["val_homography_correct_3"], row["val_repeatability"])
        if m["keep_best"] and (self.best is None or key > self.best):
            self.best = key
            self.saveModel(BEST_NAME, metrics=row)
        return row

    def saveModel(self, name=None, **extra):
        """Train_model_frontend.py:340-353 with save_checkpoint's file name (utils/utils.py:534-541); `name` and further keys are the
        best checkpoint's (validate_metrics)"""
        state = {"n_iter": self.n_iter + 1, "model_state_dict": self.net.state_dict(), "optimizer_state_dict": self.optimizer.state_dict(),
                 "loss": self.loss}
        state.update(extra)
        name = name or "{}_{}_{}".format("superPointNet", str(self.n_iter), "checkpoint.pth.tar")
        os.makedirs(str(self.save_path), exist_ok=True)
        torch.save(state, os.path.join(str(self.save_path), name))
        logging.info("save checkpoint to %s", name)
        return os.path.join(str(self.save_path), name)
