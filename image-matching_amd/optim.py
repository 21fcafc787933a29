"""The optimiser step of the training loop in the library: FlatAdam is torch.optim.Adam (amsgrad=False, maximize=False) whose step is ONE
launch of imx_adam_flat (include/imx_sploop.h) instead of a dozen `foreach` launches over 48 small tensors.

    model = SuperPointTrainable(engine, 128).train()
    optimizer = FlatAdam(model.parameters(), engine, lr=1e-4)
    loss(model(images)).backward()                   # autograd accumulates into the gradient arena in place
    optimizer.step()                                 # one kernel; it zeroes the gradients too

Four arenas of the same layout, one flat fp32 tensor each: parameters, gradients, exp_avg, exp_avg_sq.  A parameter's offset is a
multiple of 4 floats (16 bytes: the kernel's float4 form never straddles two parameters); the padding between them is 0 in all four
arenas and stays 0 (an Adam step on p = g = m = v = 0 leaves p at 0 for eps > 0).  `p.data` becomes a view of the first arena and `p.grad`
a view of the second, so nn.Parameter identity, Module.state_dict() and load_state_dict() (which copies in place) keep working.

state_dict() / load_state_dict() speak torch.optim.Adam's format: the reference's checkpoints load here and ours load there."""
import torch

from .engine import ImxError


class FlatAdam:
    def __init__(self, params, engine, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        """params: an iterable of fp32 parameters on one device (the engine's, if one is given).  engine=None builds the arenas and serves
        state_dict() / load_state_dict() / zero_grad() only; step() raises."""
        self.params = list(params)
        if not self.params:
            raise ImxError("FlatAdam: no parameters")
        if not (float(lr) >= 0 and 0 <= betas[0] < 1 and 0 <= betas[1] < 1 and float(weight_decay) >= 0):
            raise ImxError(f"FlatAdam: bad hyper-parameters lr={lr} betas={betas} weight_decay={weight_decay}")
        if not float(eps) > 0:
            raise ImxError("FlatAdam: eps must be positive (the padding between parameters is held at 0 by 0 / eps)")
        dev = self.params[0].device
        for p in self.params:
            if not isinstance(p, torch.Tensor) or p.dtype != torch.float32 or p.device != dev or not p.requires_grad or not p.is_leaf:
                raise ImxError("FlatAdam: every parameter must be a leaf fp32 tensor that requires grad, all on one device")
        if engine is not None and torch.device(engine.device) != dev:
            raise ImxError(f"FlatAdam: the parameters live on {dev}, the engine on {engine.device}")
        self.engine = engine
        self.offsets, total = [], 0
        for p in self.params:
            self.offsets.append(total)
            total += -(-p.numel() // 4) * 4
        self.numel = total
        self.p_arena, self.g_arena, self.m_arena, self.v_arena = (torch.zeros(total, dtype=torch.float32, device=dev) for _ in range(4))
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                view = self.p_arena[o:o + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view
                p.grad = self.g_arena[o:o + p.numel()].view(p.shape)
        self.step_count = 0
        # the keys and defaults of this torch's Adam, so that a state dict of ours is one of its
        template = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                                    weight_decay=float(weight_decay)).state_dict()["param_groups"][0]
        template["params"] = list(range(len(self.params)))
        self.param_groups = [template]

    # ---------------------------------------------------------------------------------------------- views
    def _views(self, arena):
        return [arena[o:o + p.numel()].view(p.shape) for p, o in zip(self.params, self.offsets)]

    def check_arenas(self):
        """every parameter and gradient still lives in its arena: a comparison of addresses on the host, no device read.  `.to()`,
        `.cuda()`, `zero_grad(set_to_none=True)` or an assignment to `.data` / `.grad` moves one out"""
        base_p, base_g = self.p_arena.data_ptr(), self.g_arena.data_ptr()
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):
            if p.device != self.p_arena.device or p.data_ptr() != base_p + 4 * o or not p.is_contiguous():
                raise ImxError(f"FlatAdam: parameter {i} {tuple(p.shape)} no longer lives in the parameter arena (moved by .to() / .cuda() or "
                               "re-assigned): build a new FlatAdam after moving a model")
            g = p.grad
            if g is None or g.device != self.g_arena.device or g.data_ptr() != base_g + 4 * o or not g.is_contiguous():
                raise ImxError(f"FlatAdam: the gradient of parameter {i} {tuple(p.shape)} no longer lives in the gradient arena "
                               "(set_to_none or re-assigned): use FlatAdam.zero_grad()")

    # ---------------------------------------------------------------------------------------------- the optimiser's interface
    def zero_grad(self, set_to_none=False):
        """one memset of the gradient arena; step() already leaves it zero, so a loop that steps every iteration need not call this"""
        if set_to_none:
            raise ImxError("FlatAdam.zero_grad: set_to_none would take the gradients out of their arena")
        self.g_arena.zero_()

    def step(self, zero_grad=True):
        """one imx_adam_flat call on the four arenas; zero_grad: the kernel stores 0 to every gradient after reading it"""
        if self.engine is None:
            raise ImxError("FlatAdam was built without an engine: there is no CPU path")
        self.check_arenas()
        g = self.param_groups[0]
        self.step_count += 1
        self.engine.adam_flat(self.p_arena, self.g_arena, self.m_arena, self.v_arena, g["lr"], g["betas"], g["eps"], g["weight_decay"],
                              self.step_count, zero_grad=zero_grad)

    def state_dict(self):
        """torch.optim.Adam's: state[i] = {step, exp_avg, exp_avg_sq} (copies), param_groups.  Before the first step the state is empty."""
        state = {}
        if self.step_count > 0:
            for i, (m, v) in enumerate(zip(self._views(self.m_arena), self._views(self.v_arena))):
                state[i] = {"step": torch.tensor(float(self.step_count)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        return {"state": state, "param_groups": [dict(g, params=list(g["params"])) for g in self.param_groups]}

    def load_state_dict(self, state_dict):
        """a state dict of torch.optim.Adam over the same parameters in the same order (one parameter group, one common step count)"""
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.params):
            raise ImxError(f"FlatAdam.load_state_dict: expected one parameter group of {len(self.params)} parameters, got "
                           f"{[len(g['params']) for g in groups]}")
        if groups[0].get("amsgrad") or groups[0].get("maximize"):
            raise ImxError("FlatAdam.load_state_dict: amsgrad and maximize are not served")
        ids = list(groups[0]["params"])
        state = state_dict["state"]
        have = [i for i in ids if i in state]
        if have and len(have) != len(ids):
            raise ImxError("FlatAdam.load_state_dict: some parameters have state and some have none: one step count serves the whole arena")
        steps = {float(state[i]["step"]) for i in have}
        if len(steps) > 1:
            raise ImxError(f"FlatAdam.load_state_dict: the parameters' step counts differ ({sorted(steps)})")
        with torch.no_grad():
            self.m_arena.zero_()
            self.v_arena.zero_()
            if have:
                for i, m, v, p in zip(ids, self._views(self.m_arena), self._views(self.v_arena), self.params):
                    if tuple(state[i]["exp_avg"].shape) != tuple(p.shape):
                        raise ImxError(f"FlatAdam.load_state_dict: state {i} has shape {tuple(state[i]['exp_avg'].shape)}, the parameter {tuple(p.shape)}")
                    m.copy_(state[i]["exp_avg"])
                    v.copy_(state[i]["exp_avg_sq"])
        self.step_count = int(steps.pop()) if steps else 0
        new = dict(self.param_groups[0])
        new.update({k: v for k, v in groups[0].items() if k != "params"})
        new["betas"] = tuple(float(b) for b in new["betas"])
        if not float(new["eps"]) > 0:
            raise ImxError("FlatAdam.load_state_dict: eps must be positive")
        self.param_groups = [new]
