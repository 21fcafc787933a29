"""The training loop's host side, no GPU: the restatement of the soft-label splat (tests/sploop_ref.py) against the fixtures the reference
wrote (tests/golden/make_golden_sploop.py), its duplicate rule on a hand-made case, the Adam restatement against torch.optim.Adam, the
fp32 restatement against the bar the kernel is held to on the GPU, FlatAdam's state dicts against torch.optim.Adam's, the sigma gate of
datasets/ALLSS_train.py, and the pins: what raised before the new modules existed still raises after they are imported."""
import os

import numpy as np
import pytest
import torch

from tests import sploop_ref as S
from tests import sptrain_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = ("120x160", "136x200")
# 20,20 and 21,20 land on one pixel; 22,20's own first corner is 20,20's third
DUP_MAT = np.array([[0.5, 0, 0.25], [0, 0.5, 0.25], [0, 0, 1]], np.float32)
DUP_PTS = np.array([[20, 20], [21.5, 20.25], [22, 20]], np.float32)
DUP_EXPECT = {(10, 10): 0.1875, (10, 11): 0.0625, (11, 10): 0.5625, (11, 11): 0.1875, (12, 10): 0.1875, (12, 11): 0.0625}     # (x, y): weight


def dup_expected(H, W, levels=0):
    out = np.zeros((H, W), np.float32)
    for (x, y), w in DUP_EXPECT.items():
        out[y, x] = w
    return S.quantise(out, levels)


@pytest.mark.parametrize("size", SIZES)
def test_restatement_equals_the_reference(size):
    fx = np.load(os.path.join(GOLDEN, f"sploop_labels_{size}.npz"))
    H, W = (int(v) for v in fx["size"])
    mats = fx["mats_px"]                                               # pixel space, as the reference scaled them where the fixture was written
    assert np.abs(R.scale_pixels(fx["homographies"], H, W) - mats).max() <= 1e-4 * np.abs(mats).max()
    counts = fx["counts"]
    assert sorted(counts.tolist()) == list(range(fx["pts"].shape[1] + 1))          # every count from 0 to Kcap
    assert (fx["coverage"] > 0).all()
    for b, n in enumerate(counts):
        bi, flag = S.labels_bi(fx["pts"][b, :n], mats[b], H, W, 0)
        assert flag == 0
        assert np.array_equal(bi.view(np.uint32), fx["labels_bi"][b].view(np.uint32)), b
        g, _ = S.labels_bi(fx["pts"][b, :n], mats[b], H, W, 255)
        assert np.array_equal(g.view(np.uint32), fx["labels_gaussian"][b].view(np.uint32)), b
        assert np.array_equal(S.quantise(fx["labels_bi"][b]).view(np.uint32), fx["labels_gaussian"][b].view(np.uint32))
        # the soft targets are fractions of 255 below the weights, and their support holds every hard label that has a non-zero weight there
        assert ((g <= bi) & (bi - g < 1 / 255)).all() and np.array_equal(np.round(g * 255), g * 255)
    assert not np.array_equal(fx["labels_bi"], fx["labels"].astype(np.float32))


def test_duplicate_rule_by_hand():
    """two points on one pixel and a point whose own corner is another's: the entry later in the reference's concatenation (k-major,
    then the point index) writes -- the values below were worked out by hand from dyadic weights"""
    out, flag = S.labels_bi(DUP_PTS, DUP_MAT, 16, 24, 0)
    assert flag == 0 and np.array_equal(out, dup_expected(16, 24))
    assert np.array_equal(S.labels_bi(DUP_PTS, DUP_MAT, 16, 24, 255)[0], dup_expected(16, 24, 255))
    # the reverse order of the points changes the winners of the shared pixels only
    rev, _ = S.labels_bi(DUP_PTS[::-1], DUP_MAT, 16, 24, 0)
    assert rev[10, 10] == np.float32(0.5625) and rev[10, 11] == np.float32(0.1875) and rev[10, 12] == out[10, 12]
    # flags: a coordinate in (-1, 0) and a zero denominator
    _, flag = S.labels_bi([[0, 4]], np.array([[1, 0, -0.5], [0, 1, 0], [0, 0, 1]], np.float32), 16, 24, 0)
    assert flag == 1
    _, flag = S.labels_bi([[3, 4]], np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0]], np.float32), 16, 24, 0)
    assert flag == 2


@pytest.mark.parametrize("t0", [0, 99999])
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_adam_restatement_float64(weight_decay, t0):
    """the float64 restatement equals torch.optim.Adam in float64 on the CPU over 5 steps (t = 1.. and t = 100 000..): per tensor,
    max |ours - torch| <= 1e-12 max |torch|"""
    case = S.adam_case(4097, 3, t0)
    ours, theirs = S.adam_run(case, weight_decay, t0, np.float64), S.adam_torch(case, weight_decay, t0, torch.float64)
    for a, b in zip(ours, theirs):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    assert np.abs(ours[-1] - case[0]).max() > 1e-4                    # the steps moved the parameters


@pytest.mark.parametrize("t0", [0, 99999])
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("n", [4097, (1 << 20) + 3])
def test_adam_fp32_restatement_meets_the_gpu_bar(n, weight_decay, t0):
    """the fp32 restatement in the header's order stays within the bar tests/test_gpu_sploop.py holds the kernel to: the bar is attainable"""
    case = S.adam_case(n, 3, t0)
    p64, bar = S.adam_bar(case, weight_decay, t0)
    p32 = S.adam_run(case, weight_decay, t0, np.float32)[-1]
    err = float(np.abs(p32.astype(np.float64) - p64).max())
    print(f"n {n} weight_decay {weight_decay} t0 {t0}: fp32 restatement {err:.3e}, bar (2 x torch fp32) {bar:.3e}, fraction {err / bar:.3f}")
    assert bar > 0 and err <= bar


def small_model(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Conv2d(1, 3, 3), torch.nn.BatchNorm2d(3), torch.nn.Conv2d(3, 5, 1))     # numels 27, 3, 3, 3, 15, 5


def test_flat_adam_state_dicts():
    from image_matching_amd.engine import ImxError
    from image_matching_amd.optim import FlatAdam
    a, b, c = small_model(0), small_model(0), small_model(0)
    opt = torch.optim.Adam(a.parameters(), lr=3e-4, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.01)
    for _ in range(2):
        for p in a.parameters():
            p.grad = torch.randn_like(p)
        opt.step()
    sd = opt.state_dict()
    fa = FlatAdam(b.parameters(), None)
    # the arenas: offsets are multiples of 4 floats, the parameters and gradients are views, the padding is zero
    assert fa.offsets == [0, 28, 32, 36, 40, 56] and fa.numel == 64
    fa.check_arenas()
    used = torch.zeros(fa.numel, dtype=torch.bool)
    for p, o in zip(fa.params, fa.offsets):
        used[o:o + p.numel()] = True
    for arena in (fa.p_arena, fa.g_arena, fa.m_arena, fa.v_arena):
        assert (arena[~used] == 0).all()
    assert fa.state_dict()["state"] == {}
    # torch.optim.Adam's state dict loads ...
    fa.load_state_dict(sd)
    assert fa.step_count == 2
    g = fa.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (3e-4, (0.8, 0.99), 1e-7, 0.01)
    mine = fa.state_dict()
    assert set(mine) == {"state", "param_groups"} and set(mine["param_groups"][0]) == set(sd["param_groups"][0])
    for i in sd["state"]:
        assert set(mine["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(mine["state"][i][k], sd["state"][i][k]), (i, k)
    for arena in (fa.m_arena, fa.v_arena):
        assert (arena[~used] == 0).all()
    # ... and ours loads into torch.optim.Adam
    opt2 = torch.optim.Adam(c.parameters())
    opt2.load_state_dict(mine)
    back = opt2.state_dict()
    assert back["param_groups"] == sd["param_groups"]
    for i in sd["state"]:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(back["state"][i][k], sd["state"][i][k]), (i, k)
    for p in c.parameters():
        p.grad = torch.randn_like(p)
    opt2.step()                                                       # torch's step runs on the loaded groups
    # a model checkpoint loaded afterwards lands in the arena: the parameters stay views
    b.load_state_dict(a.state_dict())
    fa.check_arenas()
    for p, q in zip(a.parameters(), fa._views(fa.p_arena)):
        assert torch.equal(p.data, q)
    # nn.Parameter identity and the module's own state dict still work
    assert all(p is q for p, q in zip(b.parameters(), fa.params))
    assert all(torch.equal(v, a.state_dict()[k]) for k, v in b.state_dict().items())
    # no engine: no step; a moved gradient is caught by address
    with pytest.raises(ImxError, match="without an engine"):
        fa.step()
    b.zero_grad(set_to_none=True)
    with pytest.raises(ImxError, match="gradient arena"):
        fa.check_arenas()
    with pytest.raises(ImxError, match="set_to_none"):
        fa.zero_grad(set_to_none=True)
    with pytest.raises(ImxError, match="step counts differ"):
        bad = opt.state_dict()
        bad["state"][0]["step"] = torch.tensor(7.0)
        FlatAdam(small_model(1).parameters(), None).load_state_dict(bad)


def test_flat_adam_on_the_trainable_superpoint():
    """the 48 parameter tensors of SuperPointTrainable in one arena; its checkpoint round trip keeps the views"""
    from image_matching_amd.optim import FlatAdam
    from image_matching_amd.sptrain_model import SuperPointTrainable
    m = SuperPointTrainable(None, descriptor_length=64)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    fa = FlatAdam(m.parameters(), None, lr=1e-4)
    assert len(fa.params) == 48 and all(o % 4 == 0 for o in fa.offsets)
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    other = SuperPointTrainable(None, descriptor_length=64)
    m.load_state_dict({"model_state_dict": other.state_dict()})
    fa.check_arenas()
    assert all(torch.equal(v, other.state_dict()[k]) for k, v in m.state_dict().items())


def gauss(sigma):
    return {'enable': True, 'params': {'GaussianBlur': {'sigma': sigma}}}


def test_sigma_gate():
    from image_matching_amd.datasets.ALLSS_train import ALLSSTrain, blur_defect, check_gaussian_label
    kw = dict(images=np.zeros((1, 16, 16), np.float32), points=[np.zeros((0, 2), np.float32)])
    assert abs(blur_defect(0.2) - 0.0038) < 1e-4 and blur_defect(0.2) == S.blur_defect(0.2)
    assert blur_defect(0.24) <= 0.25 < blur_defect(0.25)
    for sigma in (0.2, 0.0005, 0):
        ds = ALLSSTrain(task='train', gaussian_label=gauss(sigma), **kw)
        assert ds.gaussian_label and ds.config['gaussian_label']['enable'] is False        # stripped before the base classes saw it
        assert ALLSSTrain(task='val', gaussian_label=gauss(sigma), **kw).gaussian_label   # both tasks, as in the reference
    for cfg in (gauss(0.3), gauss((0.1, 0.2)), gauss([0.0, 0.2]), {'enable': True}, {'enable': True, 'params': {}}, gauss(None), gauss(True)):
        with pytest.raises(NotImplementedError, match=r"255 \(1 - w0\^2\) <= 0.25"):
            ALLSSTrain(task='train', gaussian_label=cfg, **kw)
        with pytest.raises(NotImplementedError):
            check_gaussian_label(cfg)
    cfg = gauss(0.2)
    ALLSSTrain(task='train', gaussian_label=cfg, **kw)
    assert cfg['enable'] is True                                       # the caller's dict is not edited
    assert not ALLSSTrain(task='train', **kw).gaussian_label and not ALLSSTrain(task='train', gaussian_label=gauss(0.3) | {'enable': False}, **kw).gaussian_label


def test_pins_after_the_new_modules_are_imported():
    import yaml
    from image_matching_amd.datasets.ALLSS import ALLSS
    from image_matching_amd.datasets.ALLSS_photo import ALLSSPhotometric
    from image_matching_amd.datasets.ALLSS_train import ALLSSTrain                                  # noqa: F401
    from image_matching_amd.superpoint import Train_model_heatmap_loop as loop
    from image_matching_amd.superpoint.Train_model_heatmap import Train_model_heatmap as Old
    from image_matching_amd.utils.photometric import ImgAugTransform
    kw = dict(images=np.zeros((1, 16, 16), np.float32), points=[np.zeros((0, 2), np.float32)])
    for cls in (ALLSS, ALLSSPhotometric):
        with pytest.raises(NotImplementedError, match="imgaug"):
            cls(task='train', gaussian_label={'enable': True}, **kw)
        with pytest.raises(NotImplementedError, match="imgaug"):
            cls(task='train', gaussian_label=gauss(0.2), **kw)
    with pytest.raises(NotImplementedError, match="imgaug"):
        ALLSS(task='train', augmentation={'photometric': {'enable': True}}, **kw)
    with pytest.raises(NotImplementedError, match="GaussianBlur"):
        ImgAugTransform(photometric={'enable': True, 'params': {'GaussianBlur': {'sigma': 0.2}}})
    with open(os.path.join(GOLDEN, "superpoint_allss_train_heatmap.yaml")) as f:
        shipped = yaml.safe_load(f)
    assert shipped['data']['gaussian_label'] == gauss(0.2) and shipped['data']['augmentation']['photometric']['enable'] is True
    with pytest.raises(NotImplementedError, match="gaussian_label"):
        Old(shipped)
    plain = yaml.safe_load(open(os.path.join(GOLDEN, "superpoint_allss_train_heatmap.yaml")))
    plain['data']['gaussian_label']['enable'] = False
    with pytest.raises(NotImplementedError, match="no backward pass"):
        Old(plain).train()
    # the new agent takes the shipped file as it is, and is the old one's subclass
    agent = loop.Train_model_heatmap(shipped, device="cuda")
    assert isinstance(agent, Old) and agent.gaussian and agent.max_iter == 100000 and shipped['data']['gaussian_label']['enable'] is True
    assert not loop.Train_model_heatmap(plain, device="cuda").gaussian
    bad = yaml.safe_load(open(os.path.join(GOLDEN, "superpoint_allss_train_heatmap.yaml")))
    bad['data']['gaussian_label']['params']['GaussianBlur']['sigma'] = 1.0
    with pytest.raises(NotImplementedError, match="w0"):
        loop.Train_model_heatmap(bad, device="cuda")
    for key, value in (("detector_loss", {"loss_type": "l2"}), ("dense_loss", {"enable": True}), ("add_res_loss", True), ("pred_soft_argmax", True)):
        cfg = yaml.safe_load(open(os.path.join(GOLDEN, "superpoint_allss_train_heatmap.yaml")))
        cfg['model'][key] = value
        with pytest.raises(NotImplementedError):
            loop.Train_model_heatmap(cfg, device="cuda")
