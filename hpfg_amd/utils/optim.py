"""Optimizer / scheduler factories with the reference's signatures (utils/__init__.py:13-49).

``build_optimizer(args, model)`` returns ``FusedSGD`` for an hpfg_amd U-Net on the GPU: torch.optim.SGD's law
(momentum, weight decay on every parameter, no dampening / nesterov) as ONE HIP kernel over the model's flat parameter,
gradient and momentum buffers, with the learning rate read from device memory so the step can live inside a hipGraph.
It is a ``torch.optim.Optimizer`` (param_groups, state_dict, zero_grad), so the reference's LR schedulers drive it unchanged.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib as L
from .scheduler import CosineWarmupLR_Scheduler, Medical_LR, PolyLR


class FusedSGD(torch.optim.Optimizer):
    def __init__(self, model, lr=0.01, momentum=0.0, weight_decay=0.0):
        self.model = model
        params = [p for p in model.parameters() if p.requires_grad]
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))
        flat = model.flat_params
        self._mom = torch.zeros_like(flat)
        self._lr_host = torch.zeros(1, dtype=torch.float32).pin_memory() if torch.cuda.is_available() else torch.zeros(1)
        self._lr_dev = torch.zeros(1, dtype=torch.float32, device=flat.device)
        self.grad_scale = 1.0
        # torch.optim.SGD skips a parameter whose .grad is None (no weight decay, no momentum).  A step that never back-propagates into a
        # trailing part of the flat buffer (HPFG's first student: its projection necks' outputs are discarded, main.py:152) says so here.
        self.active_numel = None
        self.pack_fragments = True      # False: a step whose next launch overwrites this model's weights anyway (HPFG's second student) says so
        self._pack_plan = None      # descriptors of the update launch that also writes the weight fragments (_update_pack_plan)

    def zero_grad(self, set_to_none: bool = False):
        if hasattr(self.model, "_hpfg_generic_flat"):      # a module laid out by flatten_parameters (SegFormer_Plus): see FusedAdamW.zero_grad
            for p in self.model.parameters():
                p.grad = None
            return
        self.model.zero_flat_grad()          # one memset; p.grad views stay attached
        self.model.attach_grad_views()

    def push_lr(self):
        """Stage the current lr on the device (async copy from pinned memory; capturable)."""
        self._lr_host[0] = float(self.param_groups[0]["lr"])
        self._lr_dev.copy_(self._lr_host, non_blocking=True)

    def _update_pack_plan(self, n_sgd: int, teacher, n_ema: int):
        """Descriptor table of hpfg_sgd_ema_pack_step for the engine that ran the model's last forward (and the teacher's), or None where the
        launch does not apply: not an hpfg_amd U-Net in bf16x3 math, a conv layer outside the updated range, or fragment buffers whose padding
        no pack launch has zeroed yet (a fresh engine packs once by itself).  Returns (plan, student engine, teacher engine or None)."""
        from ..engine import DescTable
        m = self.model
        eng = getattr(m, "_last_engine", None)
        if eng is None or getattr(m, "math", None) != "bf16x3" or eng.math != L.MATH_BF16X3 or not {"f", "d"} <= eng.pads_zeroed:
            return None
        if not any(eng is e for pool in m._engines.values() for e in pool):      # (the model was re-flattened: its engines are gone)
            return None
        layers = sorted(eng.packed, key=lambda s: m._offsets[f"{s.name}.weight"][0])
        end = max(sum(m._offsets[f"{s.name}.bias"]) for s in layers)
        teng = getattr(teacher, "_last_engine", None) if teacher is not None else None
        # the teacher rides along with all of its layers or not at all: same layout, every conv inside the averaged slice, padding zeroed
        if teng is not None and (teacher.math != "bf16x3" or teng.math != L.MATH_BF16X3 or "f" not in teng.pads_zeroed or end > n_ema
                                 or teacher._offsets != m._offsets or not any(teng is e for pool in teacher._engines.values() for e in pool)):
            teng = None
        key = (eng, teng, m._flat.data_ptr(), n_sgd, n_ema)
        if self._pack_plan is not None and self._pack_plan[0][0] is eng and self._pack_plan[0][1] is teng and self._pack_plan[0][2:] == key[2:]:
            return self._pack_plan[1], eng, teng
        if torch.cuda.is_current_stream_capturing():      # (the tables are copied to the device when they are built: not inside a capture)
            return None
        descs =(L.UpdatePackDesc * len(layers))()
        gaps, at = [], 0
        for d, s in zip(descs, layers):
            (wo, wn), (bo, bn) = m._offsets[f"{s.name}.weight"], m._offsets[f"{s.name}.bias"]
            if not (at <= wo and wo + wn <= bo and bo + bn <= n_sgd):
                return None
            d.w_off, d.b_off = wo, bo
            d.wpk16_fwd, d.wpk16_dgrad, d.bias_pad = L.ptr(eng.wpk16_f[s.name]), L.ptr(eng.wpk16_d[s.name]), L.ptr(eng.bias_pad[s.name])
            if teng is not None:
                d.t_wpk16_fwd, d.t_bias_pad = L.ptr(teng.wpk16_f[s.name]), L.ptr(teng.bias_pad[s.name])
            d.Cout, d.Cin, d.CoutPad, d.CinPad, d.taps = s.cout, s.cin, s.cout_pad, s.cin_pad, s.taps
            d.kc, d.kc_t = eng.kc[s.name], (teng or eng).kc[s.name]
            for lo, hi in ((at, wo), (wo + wn, bo)):
                if hi > lo:
                    gaps.append((lo, hi))
            at = bo + bn
        if at < n_sgd:
            gaps.append((at, n_sgd))
        gh = (C.c_long * (2 * max(len(gaps), 1)))(*[v for g_ in gaps for v in g_])
        gd = torch.tensor([v for g_ in gaps for v in g_] or [0, 0], dtype=torch.int64).to(m._flat.device)
        plan = (DescTable(descs, m._flat.device), gh, gd, len(gaps))
        self._pack_plan = (key, plan)
        return plan, eng, teng

    @torch.no_grad()
    def step(self, closure=None, push_lr: bool = True, ema=None):
        """ema: optional (teacher_flat, numel, alpha_dev[, teacher model]) -- the EMA teacher update of the same iteration rides along in the
        same launch (hpfg_sgd_ema_step; bit-identical to step() followed by utils.update_ema_variables).  On an hpfg_amd U-Net in bf16x3 math
        the launch also writes the weight fragments the next forward reads (hpfg_sgd_ema_pack_step: same update, bit for bit), for the engine
        of the model's last forward and -- with the teacher model given -- the teacher's; every other engine of either model goes stale."""
        g = self.param_groups[0]
        if hasattr(self.model, "_hpfg_generic_flat"):
            gather_flat_grads(self.model, self.active_numel)
        flat, grad = self.model.flat_params, self.model.flat_grads
        if self._mom.data_ptr() == 0 or self._mom.numel() != flat.numel() or self._mom.device != flat.device:
            self._mom = torch.zeros_like(flat)
        if push_lr:
            self.push_lr()
        st = torch.cuda.current_stream(flat.device).cuda_stream
        n_sgd = flat.numel() if self.active_numel is None else int(self.active_numel)
        lib = L.load()
        teacher = ema[3] if ema is not None and len(ema) > 3 else None
        for m in (self.model, teacher):      # raw-pointer writes: torch's version counters do not see them
            if hasattr(m, "mark_fragments_stale"):
                m.mark_fragments_stale()
        if ema is not None:
            assert ema[0].is_cuda and ema[0].dtype == torch.float32 and ema[0].numel() == flat.numel() and 0 <= ema[1] <= n_sgd
        found = self._update_pack_plan(n_sgd, teacher, int(ema[1]) if ema is not None else 0) if (
            self.pack_fragments and lib.hpfg_get_option(L.OPT_UPDATE_PACK) != 0 and hasattr(self.model, "_engines")) else None
        if found is not None:
            (table, gaps_host, gaps_dev, ngaps), eng, teng = found
            dev, host, nl = table.sub(0, len(table.host))
            t, n_ema, alpha_dev = (ema[0], int(ema[1]), ema[2]) if ema is not None else (None, 0, None)
            L.check(lib.hpfg_sgd_ema_pack_step(L.ptr(flat), L.ptr(grad), L.ptr(self._mom), n_sgd, L.ptr(self._lr_dev), float(g["momentum"]),
                                               float(g["weight_decay"]), float(self.grad_scale), L.ptr(t), n_ema, L.ptr(alpha_dev), dev, host, nl,
                                               L.ptr(gaps_dev), gaps_host, ngaps, st), "sgd_ema_pack_step")
            eng.frag_token, eng.frag_dgrad = self.model._weights_token(), True
            if teng is not None:
                teng.frag_token, teng.frag_dgrad = teacher._weights_token(), False
            return
        if ema is not None:
            t, n_ema, alpha_dev = ema[:3]
            L.check(L.load().hpfg_sgd_ema_step(L.ptr(flat), L.ptr(grad), L.ptr(self._mom), n_sgd, L.ptr(self._lr_dev), float(g["momentum"]),
                                               float(g["weight_decay"]), float(self.grad_scale), L.ptr(t), int(n_ema), L.ptr(alpha_dev), st),
                    "sgd_ema_step")
            return
        L.check(L.load().hpfg_sgd_step(L.ptr(flat), L.ptr(grad), L.ptr(self._mom), n_sgd, L.ptr(self._lr_dev), float(g["momentum"]),
                                       float(g["weight_decay"]), float(self.grad_scale), st), "sgd_step")

    def state_dict(self):
        d = super().state_dict()
        d["flat_momentum"] = self._mom
        return d

    def load_state_dict(self, sd):
        sd = dict(sd)
        mom = sd.pop("flat_momentum", None)
        super().load_state_dict(sd)
        if mom is not None:
            self._mom.copy_(mom)


def flat_order(model):
    """The order in which ``flatten_parameters`` lays a module's parameters into its flat buffer: ``parameters()`` order with the frozen ones
    (requires_grad False) moved behind the trainable ones when a module has both -- a frozen parameter gets no gradient and must not be
    stepped or decayed, and the flat kernels can only leave out a trailing range (``active_numel``).  A module whose parameters are all
    trainable, or all frozen (an EMA teacher), keeps ``parameters()`` order.  Swin-MAE's ``pos_embed`` is the one mixed case."""
    ps = list(model.parameters())
    return [p for p in ps if p.requires_grad] + [p for p in ps if not p.requires_grad]


def flatten_parameters(model):
    """Re-point every parameter of `model` at a slice of ONE flat fp32 buffer (gradients are packed into a second flat buffer per step), so
    that an optimizer step is a single kernel.  The hpfg_amd U-Nets are built that way; this does it for any module (SegFormer).
    Must run after the module is on its device.  Sets model.flat_params / model.flat_grads."""
    if hasattr(model, "flat_params"):
        return
    ps = flat_order(model)
    dev = ps[0].device
    n = sum(p.numel() for p in ps)
    flat = torch.empty(n, dtype=torch.float32, device=dev)
    grad = torch.zeros(n, dtype=torch.float32, device=dev)
    o = 0
    with torch.no_grad():
        for p in ps:
            k = p.numel()
            flat[o:o + k].copy_(p.detach().reshape(-1))
            p.data = flat[o:o + k].view(p.shape)
            o += k
    model.flat_params, model.flat_grads = flat, grad
    model._hpfg_flat_order = ps          # the layout, whatever happens to requires_grad afterwards (gather_flat_grads packs in this order)
    model._hpfg_generic_flat = True      # gradients reach flat_grads only through FusedAdamW.gather_flat_grads()


@torch.no_grad()
def gather_flat_grads(model, active_numel=None):
    """Pack the per-parameter gradients autograd left on a ``flatten_parameters`` module into ``model.flat_grads`` with ONE concat.
    active_numel: only the leading parameters that make up that many elements -- the rest of the buffer is neither written here nor read
    by the optimizer kernels.

    Every parameter of the packed range must hold a gradient.  torch.optim.SGD / AdamW skip a parameter whose ``.grad`` is None (no weight
    decay, no moment update); the flat kernels cannot skip a slice in the middle, and a gradient of zeros is NOT the same: the weight would
    still decay and the moments shrink.  No module of this package has such a parameter: SegFormer, SegFormer_Plus and the Swin blocks
    use every parameter they construct in every forward (``sr`` / ``norm`` of an Attention exist only where sr_ratio > 1, a
    BasicBlock's ``downsample`` only where it is applied; a dropped path yields a zero gradient, not a missing one), and the one trailing
    group a step leaves out -- the necks of HPFG's first student -- is cut off by active_numel.  Anything else is refused."""
    ps, k = [], 0
    for p in getattr(model, "_hpfg_flat_order", None) or list(model.parameters()):
        if active_numel is not None and k >= active_numel:
            break
        ps.append(p)
        k += p.numel()
    assert active_numel is None or k == active_numel, "active_numel must end on a parameter boundary"
    missing = [i for i, p in enumerate(ps) if p.grad is None]
    if missing:
        ids = {id(ps[i]) for i in missing}
        names = [n for n, p in model.named_parameters() if id(p) in ids]
        raise RuntimeError(f"gather_flat_grads: {len(missing)} parameter(s) inside the updated range have no gradient ({', '.join(names[:4])}"
                           f"{', ...' if len(names) > 4 else ''}): torch's optimizers would skip them, the flat kernels would decay them. "
                           "Lay parameters that a step leaves out at the end of the module and set the optimizer's active_numel")
    out = model.flat_grads if active_numel is None else model.flat_grads[:k]
    torch.cat([p.grad.reshape(-1) for p in ps], out=out)
    return model.flat_grads


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW(lr, weight_decay) -- betas (0.9, 0.999), eps 1e-8 as the reference leaves them (utils/__init__.py:17-19) -- as ONE
    HIP kernel over the model's flat parameter / gradient / moment buffers; learning rate and step count live on the device, so the
    update replays inside a hipGraph.  A ``torch.optim.Optimizer`` (param_groups, zero_grad), so the LR schedulers drive it unchanged."""

    def __init__(self, model, lr=1e-3, weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-8):
        flatten_parameters(model)
        self.model = model
        super().__init__([p for p in model.parameters() if p.requires_grad], dict(lr=lr, weight_decay=weight_decay, betas=betas, eps=eps))
        flat = model.flat_params
        self._m, self._v = torch.zeros_like(flat), torch.zeros_like(flat)
        self._step_dev = torch.zeros(1, dtype=torch.float32, device=flat.device)
        self._lr_host = torch.zeros(1, dtype=torch.float32).pin_memory()
        self._lr_dev = torch.zeros(1, dtype=torch.float32, device=flat.device)
        self.grad_scale = 1.0
        # WHO packs the per-parameter gradients into model.flat_grads is a property of the step object, fixed when it is built -- not a
        # per-call flag: a captured step evaluates host flags once, at capture time (round-4 advisor finding: graph_b captured step() with
        # the flag False, so every replay re-concatenated the UN-reduced p.grad over the all-reduced buffer).  external_gather = True
        # (data parallel: _StepBase._own_gather): the gradient exchange gathers, reduces in place, and step() consumes flat_grads as they
        # are; False (one rank): step() gathers.
        self.external_gather = False
        # torch.optim.AdamW skips a parameter whose .grad is None: no moment update, no step, and no weight decay either.  A step that never
        # back-propagates into a trailing part of the flat buffer (HPFG's first student: its necks) says so here, as on FusedSGD.
        self.active_numel = None
        n_train = sum(p.numel() for p in model.parameters() if p.requires_grad)
        if 0 < n_train < flat.numel():          # frozen parameters lie behind the trainable ones (flat_order): the update stops in front of them
            self.active_numel = n_train
        model._hpfg_flat_optimizer = self

    def zero_grad(self, set_to_none: bool = True):
        # grads are dropped, not zeroed: autograd then ASSIGNS each parameter's gradient (accumulating into kept views would cost one
        # add kernel per parameter tensor, 189 launches); gather_flat_grads() packs them into the flat buffer in one concat
        for p in self.model.parameters():
            p.grad = None

    def gather_flat_grads(self):
        return gather_flat_grads(self.model, self.active_numel)

    def push_lr(self):
        self._lr_host[0] = float(self.param_groups[0]["lr"])
        self._lr_dev.copy_(self._lr_host, non_blocking=True)

    @torch.no_grad()
    def step(self, closure=None, push_lr: bool = True):
        g = self.param_groups[0]
        flat = self.model.flat_params
        grad = self.model.flat_grads if self.external_gather else self.gather_flat_grads()
        if push_lr:
            self.push_lr()
        st = torch.cuda.current_stream(flat.device).cuda_stream
        n = flat.numel() if self.active_numel is None else int(self.active_numel)
        L.check(L.load().hpfg_adamw_step(L.ptr(flat), L.ptr(grad), L.ptr(self._m), L.ptr(self._v), n, L.ptr(self._lr_dev), L.ptr(self._step_dev),
                                         float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]), float(self.grad_scale), st),
                "adamw_step")
        if hasattr(self.model, "mark_fragments_stale"):      # a write through raw pointers (FusedSGD.step)
            self.model.mark_fragments_stale()

    def state_dict(self):
        """torch's dict plus the flat Adam moments and the device step count (resuming must not reset them; the reference saves
        ``optimizer.state_dict()`` in its checkpoints, main.py:262-272)."""
        d = super().state_dict()
        d["flat_m"], d["flat_v"], d["step"] = self._m, self._v, self._step_dev
        return d

    def load_state_dict(self, sd):
        sd = dict(sd)
        m, v, st = sd.pop("flat_m", None), sd.pop("flat_v", None), sd.pop("step", None)
        super().load_state_dict(sd)
        if m is not None:
            self._m.copy_(m)
        if v is not None:
            self._v.copy_(v)
        if st is not None:
            self._step_dev.copy_(torch.as_tensor(st, dtype=torch.float32).reshape(1))


def build_optimizer(args, model):
    if args.opt == "sgd":
        if hasattr(model, "flat_params") and model.flat_params.is_cuda:
            return FusedSGD(model, lr=args.lr, momentum=args.momentum, weight_decay=args.weight_decay)
        return torch.optim.SGD(model.parameters(), lr=args.lr, momentum=args.momentum, weight_decay=args.weight_decay)
    if args.opt == "adamW":
        params = list(model.parameters())
        if params and params[0].is_cuda:
            return FusedAdamW(model, lr=args.lr, weight_decay=args.weight_decay)
        return torch.optim.AdamW(params, lr=args.lr, weight_decay=args.weight_decay)
    if args.opt == "adam":
        return torch.optim.Adam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    raise ValueError("get_optimizer error")


def build_lr_scheduler(args, optimizer):
    if args.sched == "cosine":
        return CosineWarmupLR_Scheduler(optimizer=optimizer, base_lr=args.lr, warmup_epochs=args.warmup_epochs, warmup_lr=args.warmup_lr,
                                        final_lr=args.min_lr, iter_per_epoch=args.step_size, num_epochs=args.total_itrs // args.step_size)
    if args.sched == "poly":
        return PolyLR(optimizer, max_iters=args.total_itrs, power=0.1, min_lr=args.min_lr)
    if args.sched == "medical":
        return Medical_LR(optimizer=optimizer, base_lr=args.lr, max_iterations=args.total_itrs)
    raise ValueError("get_lr_scheduler error")
