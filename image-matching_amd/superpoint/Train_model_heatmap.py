"""Drop-in for the reference's descriptor-training agent (superpoint/Train_model_heatmap.py:33-430), forward VALUE only: one
validation pass of train_val_sample (:83-314) -- loss_det, loss_det_warp, loss_desc, positive / negative distances, precision and
recall -- on one stream without a host synchronisation.  There is no backward pass, so `train()` raises; the optimiser step stays
with the reference.  Served: detector_loss.loss_type 'softmax' and sparse_loss (the shipped yaml); not served: 'l2', dense_loss,
add_res_loss / pred_soft_argmax, tensorboard, checkpoints."""
from pathlib import Path

import torch

from .. import _lib as L
from .. import sptrain
from .loss_functions.sparse_loss import batch_descriptor_loss_sparse
from .models.superpoint_train import SuperPoint

NO_BACKWARD = ("image_matching_amd serves descriptor training up to the forward value of the objective: there is no backward pass, "
               "so the optimiser step stays with the reference (use val_sample for a validation pass)")


class Train_model_heatmap(object):
    default_config = {"train_iter": 170000, "save_interval": 2000, "tensorboard_interval": 200,
                      "model": {"subpixel": {"enable": False}}, "data": {"gaussian_label": {"enable": False}}}

    def __init__(self, config, save_path=Path("."), device="cuda", verbose=False):
        self.config = config
        self.device = device
        self.save_path = save_path
        self.cell_size = 8
        model = config["model"]
        if config.get("data", {}).get("gaussian_label", {}).get("enable"):
            raise NotImplementedError("gaussian_label needs imgaug's GaussianBlur on the host, which this project does not restate")
        if model.get("dense_loss", {}).get("enable"):
            raise NotImplementedError("dense_loss is not served: only sparse_loss (the shipped yaml)")
        if not model.get("sparse_loss", {}).get("enable"):
            raise NotImplementedError("sparse_loss must be enabled: it is the descriptor loss this project serves")
        if model.get("detector_loss", {}).get("loss_type", "softmax") != "softmax":
            raise NotImplementedError("detector_loss.loss_type 'l2' is not served: only 'softmax' (the shipped yaml)")
        self.desc_params = dict(model["sparse_loss"]["params"])
        self.descriptor_loss = batch_descriptor_loss_sparse
        self.desc_loss_type = "sparse"
        self.net = None
        self.scalar_dict = {}

    def loadModel(self, state_dict=None):
        """The dense SuperPoint (superpoint_train.SuperPoint); without a state dict it keeps its synthetic weights."""
        self.net = SuperPoint(self.config["model"].get("descriptor_length", 256)).to(self.device)
        if state_dict is not None:
            self.net.load_state_dict(state_dict)
        return self.net

    def dataParallel(self):
        return self.net

    def train(self, **options):
        raise NotImplementedError(NO_BACKWARD)

    def detector_loss(self, input, target, mask=None, loss_type="softmax"):
        """input: semi (B,65,Hc,Wc); target: labels_2D (B,1,H,W) and mask: mask_2D (B,1,H,W) -- the fused kernel does labels2Dto3D
        and getMasks itself, so it takes the 2-D maps the reference builds its 3-D targets from."""
        if loss_type != "softmax":
            raise NotImplementedError("detector_loss: loss_type 'l2' is not served, only 'softmax' (the shipped yaml)")
        if target.dim() == 4 and target.shape[1] == 65:
            raise ValueError("detector_loss takes labels_2D (B,1,H,W), not the 65-channel target: the kernel forms it per cell")
        eng = sptrain.plain_engine(input.device, self.config["model"].get("descriptor_length", 256))
        if mask is None:
            mask = torch.ones_like(target)
        return eng.detector_loss(input, target, mask)[0]

    @staticmethod
    def batch_precision_recall(batch_pred, batch_labels):
        """precisionRecall_torch (utils/utils.py:521-532) per image, then the means: device tensors, nothing read back."""
        B = batch_labels.shape[0]
        pred, labels = batch_pred.reshape(B, -1).float(), batch_labels.reshape(B, -1).float()
        tp = (pred * labels).sum(1)
        return {"precision": (tp / (pred.sum(1) + 1e-6)).mean(), "recall": (tp / (labels.sum(1) + 1e-6)).mean()}

    def heatmap_to_nms(self, eng, heatmap):
        """heatmap_nms (:413-422) for a batch: getPtsFromHeatmap on each map, the points scattered into a 0/1 map (B,H,W)."""
        B, H, W = heatmap.shape[0], heatmap.shape[-2], heatmap.shape[-1]
        m = self.config["model"]
        rows = [eng.heatmap_points(heatmap[b], m.get("detection_threshold", 0.015), m.get("nms", 4)) for b in range(B)]
        cap = rows[0][0].shape[0]
        pts = torch.stack([r[0][:, :2] for r in rows]).contiguous()
        counts = torch.clamp(torch.cat([r[1] for r in rows]), max=cap)
        return eng.warp_labels(pts, counts, None, H, W, want_res=False)[0]

    def val_sample(self, sample, generator=None, grads=False):
        """One validation batch: `sample` is ALLSS.batch(indices).  Returns the scalar dictionary of train_val_sample (:251-259, :305-309)
        as 0-d device tensors.  grads=True: the losses run as value-and-gradient calls (Engine.sp_train_loss_grads) and the dictionary
        also holds the L2 norms of d loss / d semi, semi_warp, desc and desc_warp."""
        if self.net is None:
            self.loadModel()
        eng = self.net._shared.get_engine([L.NET_SUPERPOINT])
        p = self.desc_params
        images = sample["image"]
        B, H, W = images.shape[0], images.shape[-2], images.shape[-1]
        choice, non = sptrain.draw(eng, sample["homographies"], H // 8, W // 8, int(p.get("num_matching_attempts", 1000)),
                                   int(p.get("num_masked_non_matches_per_match", 10)), generator)
        losses = eng.sp_train_loss_grads if grads else eng.sp_train_losses
        out = losses(images, sample["pts"], sample["counts"], sample["homographies"], sample["inv_homographies"], choice, non,
                     erosion_radius=sample.get("valid_border_margin", 0), lamda_d=p.get("lamda_d", 250), method=p.get("method", "1d"),
                     lambda_loss=self.config["model"].get("lambda_loss", 1))
        pred = self.heatmap_to_nms(eng, eng.superpoint_heatmap(images.reshape(B, 1, H, W).to(eng.device, torch.float32)))
        self.scalar_dict = {k: out[k] for k in ("loss", "loss_det", "loss_det_warp", "positive_dist", "negative_dist")}
        self.scalar_dict.update(self.batch_precision_recall(pred, out["labels_2D"]))
        if grads:
            self.scalar_dict.update({k + "_norm": out[k].norm() for k in ("grad_semi", "grad_semi_warp", "grad_desc", "grad_desc_warp")})
        self.outputs = out
        return self.scalar_dict
