"""GPU: the optimizer's update launch that also writes the weight fragments (hpfg_sgd_ema_pack_step, csrc/update_pack.hip) and the
staleness rule that lets a forward start without a pack launch (UNetEngine.frag_token).  Everything is bitwise:
the launch replaces hpfg_sgd_ema_step / hpfg_sgd_step + hpfg_pack_weights and must leave the same bits in every buffer.

The kernel-level cases are driven by the layer table alone (channel counts and kc, the K packing of hpfg_conv_kc), so the 24 x 24 case --
kc = 32 in every layer -- runs there although the model itself takes only inputs that are multiples of 16."""
import pytest
import torch

from hpfg_amd import _lib as L
from hpfg_amd import engine as E
from hpfg_amd.datasets.synthetic import synth_batch
from hpfg_amd.engine import MarkLog
from hpfg_amd.model import UNet, reset_dropout_streams
from hpfg_amd.train import CPSStep, GraphedStep, MeanTeacherStep, SupervisedStep, batch_pair
from tests.dp_rank_worker import _frozen, opt_args
from tests.helpers import stream

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = [(1, 4, 32), (1, 4, 24), (3, 2, 32), (1, 9, 32)]      # (input channels, classes, input height = width)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- kernel level ---------------------------------------------------------------------------------------------------------------------
class _Frags:
    """Fragment buffers and padded bias rows of every packed layer, as an engine allocates them."""

    def __init__(self, layers, kc):
        lib = L.load()
        self.f = {s.name: torch.empty(lib.hpfg_wpk16_elems(s.cin, s.cout_pad, s.taps, kc[s.name]), dtype=torch.bfloat16, device=DEV) for s in layers}
        self.d = {s.name: torch.empty(lib.hpfg_wpk16_elems(s.cout, s.cin_pad, s.taps, kc[s.name]), dtype=torch.bfloat16, device=DEV) for s in layers}
        self.b = {s.name: torch.empty(s.cout_pad, device=DEV) for s in layers}

    def pack(self, flat, offsets, layers, kc, dgrad):
        """hpfg_pack_weights (bf16x3 layouts) from the weights in `flat`."""
        d = (L.PackDesc * len(layers))()
        for q, s in zip(d, layers):
            q.w_oihw, q.b = flat.data_ptr() + 4 * offsets[s.name + ".weight"][0], flat.data_ptr() + 4 * offsets[s.name + ".bias"][0]
            q.bias_pad, q.wpk16_fwd, q.wpk16_dgrad, q.kc = L.ptr(self.b[s.name]), L.ptr(self.f[s.name]), L.ptr(self.d[s.name]) if dgrad else None, kc[s.name]
            q.Cout, q.Cin, q.CoutPad, q.CinPad, q.taps = s.cout, s.cin, s.cout_pad, s.cin_pad, s.taps
        tab = torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8).to(DEV)
        L.check(L.load().hpfg_pack_weights(tab.data_ptr(), d, len(layers), stream(DEV)), "pack")
        torch.cuda.synchronize()


def _fused(p, g, mom, t, alpha, lr, offsets, layers, kc, sf, tf):
    """hpfg_sgd_ema_pack_step over the whole flat buffer; sf / tf: the student's / the teacher's _Frags (tf None: no teacher)."""
    import ctypes as C
    n = p.numel()
    layers = sorted(layers, key=lambda s: offsets[s.name + ".weight"][0])
    d = (L.UpdatePackDesc * len(layers))()
    gaps, at = [], 0
    for q, s in zip(d, layers):
        (wo, wn), (bo, bn) = offsets[s.name + ".weight"], offsets[s.name + ".bias"]
        q.w_off, q.b_off = wo, bo
        q.wpk16_fwd, q.wpk16_dgrad, q.bias_pad = L.ptr(sf.f[s.name]), L.ptr(sf.d[s.name]), L.ptr(sf.b[s.name])
        if tf is not None:
            q.t_wpk16_fwd, q.t_bias_pad = L.ptr(tf.f[s.name]), L.ptr(tf.b[s.name])
        q.Cout, q.Cin, q.CoutPad, q.CinPad, q.taps, q.kc, q.kc_t = s.cout, s.cin, s.cout_pad, s.cin_pad, s.taps, kc[s.name], kc[s.name]
        gaps += [r for r in ((at, wo), (wo + wn, bo)) if r[1] > r[0]]
        at = bo + bn
    if at < n:
        gaps.append((at, n))
    flat_gaps = [v for r in gaps for v in r]
    gh = (C.c_long * len(flat_gaps))(*flat_gaps)
    gd = torch.tensor(flat_gaps, dtype=torch.int64).to(DEV)
    tab = torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8).to(DEV)
    L.check(L.load().hpfg_sgd_ema_pack_step(L.ptr(p), L.ptr(g), L.ptr(mom), n, L.ptr(lr), 0.9, 1e-4, 0.5, L.ptr(t), n if t is not None else 0,
                                            L.ptr(alpha) if t is not None else None, tab.data_ptr(), d, len(layers), gd.data_ptr(), gh, len(gaps),
                                            stream(DEV)), "sgd_ema_pack_step")
    torch.cuda.synchronize()


@pytest.mark.parametrize("teacher", [True, False])
@pytest.mark.parametrize("in_ch,ncls,hw", CASES)
def test_fused_update_equals_update_then_pack_bitwise(in_ch, ncls, hw, teacher):
    """hpfg_sgd_ema_step (or, without a teacher, hpfg_sgd_step) followed by hpfg_pack_weights == hpfg_sgd_ema_pack_step: every flat buffer,
    every fragment buffer (student fwd and dgrad, teacher fwd) and every padded bias row, bit for bit.  The fused launch writes weight
    positions only, so its buffers are first packed from OTHER weights: a position it misses keeps a wrong value, the padding its zeros."""
    lib = L.load()
    torch.manual_seed(5)
    offsets = UNet(in_ch, ncls)._offsets
    layers = [s for s in E.build_specs(in_ch, ncls, hw, hw).values() if s.idx > 0]
    kc = {s.name: lib.hpfg_conv_kc(s.h, s.w, s.taps) for s in layers}
    if hw == 24:
        assert set(kc.values()) == {32}
    elif in_ch == 1 and ncls == 4:
        assert set(kc.values()) == {16, 32}
    n = sum(k for _, k in offsets.values())
    g = torch.Generator().manual_seed(11)
    w0, gr, m0, t0, other = ((torch.randn(n, generator=g) * sc).to(DEV) for sc in (0.2, 1.0, 0.3, 0.2, 0.2))
    lr, alpha = torch.tensor([0.05], device=DEV), torch.tensor([0.97], device=DEV)
    st = stream(DEV)
    # reference: the separate launches
    pa, ma, ta = w0.clone(), m0.clone(), t0.clone()
    if teacher:
        L.check(lib.hpfg_sgd_ema_step(L.ptr(pa), L.ptr(gr), L.ptr(ma), n, L.ptr(lr), 0.9, 1e-4, 0.5, L.ptr(ta), n, L.ptr(alpha), st), "sgd_ema")
    else:
        L.check(lib.hpfg_sgd_step(L.ptr(pa), L.ptr(gr), L.ptr(ma), n, L.ptr(lr), 0.9, 1e-4, 0.5, st), "sgd")
    sa, tfa = _Frags(layers, kc), _Frags(layers, kc)
    sa.pack(pa, offsets, layers, kc, True)
    tfa.pack(ta, offsets, layers, kc, False)
    # fused
    pb, mb, tb = w0.clone(), m0.clone(), t0.clone()
    sb, tfb = _Frags(layers, kc), _Frags(layers, kc)
    sb.pack(other, offsets, layers, kc, True)
    tfb.pack(other, offsets, layers, kc, False)
    _fused(pb, gr, mb, tb if teacher else None, alpha, lr, offsets, layers, kc, sb, tfb if teacher else None)
    assert _same(pa, pb) and _same(ma, mb) and _same(ta, tb)
    assert not _same(pa, w0) and (not teacher or not _same(ta, t0))
    for s in layers:
        assert _same(sa.f[s.name], sb.f[s.name]), ("student fwd", s.name)
        assert _same(sa.d[s.name], sb.d[s.name]), ("student dgrad", s.name)
        assert _same(sa.b[s.name], sb.b[s.name]), ("student bias", s.name)
        if teacher:
            assert _same(tfa.f[s.name], tfb.f[s.name]), ("teacher fwd", s.name)
            assert _same(tfa.b[s.name], tfb.b[s.name]), ("teacher bias", s.name)


def test_fused_update_refuses_tables_that_do_not_tile_the_buffer():
    """Descriptors and gaps must cover every element exactly once: a missing gap is an argument error, not a launch."""
    lib = L.load()
    offsets = UNet(1, 4)._offsets
    layers = [s for s in E.build_specs(1, 4, 32, 32).values() if s.idx > 0]
    kc = {s.name: lib.hpfg_conv_kc(s.h, s.w, s.taps) for s in layers}
    n = sum(k for _, k in offsets.values())
    p, gr, mom = (torch.zeros(n, device=DEV) for _ in range(3))
    lr = torch.tensor([0.05], device=DEV)
    fr = _Frags(layers, kc)
    offsets = dict(offsets)
    wo, wn = offsets[layers[3].name + ".weight"]
    offsets[layers[3].name + ".weight"] = (wo + 1, wn)      # the gap list built from these offsets no longer matches the buffer
    with pytest.raises(L.HipLibraryError):
        _fused(p, gr, mom, None, None, lr, offsets, layers, kc, fr, None)
    assert float(p.abs().max()) == 0.0


# ---- step level -----------------------------------------------------------------------------------------------------------------------
class _Option:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = L.load().hpfg_set_option(L.OPT_UPDATE_PACK, self.value)

    def __exit__(self, *a):
        L.load().hpfg_set_option(L.OPT_UPDATE_PACK, self.old)


def _masks(seed, n):
    """Explicit dropout keep masks of the five encoder sites (uint8 NHWC), so that two models draw the same ones."""
    g = torch.Generator().manual_seed(seed)
    return {E.enc_prefix(lvl) + ".0": (torch.rand(n, 32 >> lvl, 32 >> lvl, E.WIDTHS[lvl], generator=g) > E.ENC_DROPOUT[lvl]).to(torch.uint8).to(DEV)
            for lvl in range(5)}


def _inputs():
    xl, yl = synth_batch(3, 2, 32, 32, 1, 4, 8)
    xu, _ = synth_batch(4, 2, 32, 32, 1, 4, 8)
    xl, xu = batch_pair(xl.to(DEV), xu.to(DEV))
    return [xl, yl.to(DEV), xu]


def _build(kind):
    reset_dropout_streams()
    torch.manual_seed(7)
    inputs = _inputs()
    if kind == "mt":
        m = UNet(1, 4).to(DEV)
        ema = _frozen(m)
        m.train()
        return MeanTeacherStep(m, ema, opt_args(), None), [m, ema], inputs
    if kind == "sup":
        m = UNet(1, 4).to(DEV)
        m.train()
        return SupervisedStep(m, opt_args(), None), [m], inputs[:2]
    m1, m2 = UNet(1, 4).to(DEV), UNet(1, 4).to(DEV)
    m1.train()
    m2.train()
    args = opt_args()
    args.model1, args.model2 = opt_args(), opt_args()
    return CPSStep(m1, m2, args, None), [m1, m2], inputs


def _run(kind, steps, option, graph_from=None):
    """`steps` iterations in train mode (dropout seeds drawn by the models); from iteration graph_from on as hipGraph replays.
    -> (every returned tensor of every iteration, every model's state_dict, did the last forward of every engine go without a pack)."""
    with _Option(option):
        st, models, inputs = _build(kind)
        outs, runner = [], None
        for it in range(1, steps + 1):
            if graph_from is not None and it >= graph_from:
                if runner is None:
                    runner = GraphedStep(st, inputs, warmup=0, alias_inputs=True)
                r = runner.step(inputs, it)
            else:
                r = st.step(*inputs, it)
            outs.append({k: v.detach().clone() for k, v in r.items() if torch.is_tensor(v)})
        torch.cuda.synchronize()
        sds = [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in models]
        nopack = [not e.last_fwd_packed for m in models for pool in m._engines.values() for e in pool]
    return outs, sds, nopack


def _assert_runs_equal(a, b):
    for i, (ra, rb) in enumerate(zip(a[0], b[0])):
        assert ra.keys() == rb.keys() and len(ra) >= 2
        for k in ra:
            assert _same(ra[k], rb[k]), (i + 1, k)
    for sa, sb in zip(a[1], b[1]):
        assert sa.keys() == sb.keys() and any(k.endswith("num_batches_tracked") for k in sa)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(kind, steps, option, graph_from=None):
        key = (kind, steps, option, graph_from)
        if key not in cache:
            cache[key] = _run(*key)
        return cache[key]
    return get


@pytest.mark.parametrize("kind,steps", [("mt", 3), ("sup", 2), ("cps", 2)])
def test_steps_with_and_without_the_fused_update_agree_bitwise(runs, kind, steps):
    """Mean-Teacher (three steps), supervised and CPS steps: option on against option off -- every returned tensor of every iteration and
    every state_dict, num_batches_tracked included.  With the option on the forwards after the first go without a pack launch."""
    on, off = runs(kind, steps, 1), runs(kind, steps, 0)
    assert all(on[2]) and not any(off[2]), (on[2], off[2])
    _assert_runs_equal(on, off)


@pytest.mark.parametrize("kind,steps", [("mt", 3), ("sup", 2), ("cps", 2)])
def test_captured_steps_equal_eager_steps_under_the_fused_update(runs, kind, steps):
    """The same iterations with every one after the first replayed from a hipGraph captured WITHOUT pack launches."""
    eager, graphed = runs(kind, steps, 1), runs(kind, steps, 1, 2)
    assert all(graphed[2])
    _assert_runs_equal(graphed, eager)


# ---- staleness ------------------------------------------------------------------------------------------------------------------------
def _other_weights():
    torch.manual_seed(23)
    return {k: v.detach().clone() for k, v in UNet(1, 4).state_dict().items()}


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("write", ["load_state_dict", "data_mul"])
def test_foreign_weight_writes_make_the_next_forward_pack_again(write, graph):
    """After two steps the student's weights are written behind the optimizer's back: load_state_dict with other weights, or
    ``p.data.mul_(0.5)`` on one conv weight.  The student's logits of the next step must equal, bitwise, the train-mode forward of a FRESH
    model holding those weights (same explicit dropout masks) -- eager, and through a GraphedStep captured before the write."""
    with _Option(1):
        st, (m, ema), inputs = _build("mt")
        masks = _masks(31, 4)
        m.external_dropout_masks, ema.external_dropout_masks = masks, _masks(32, 4)
        st.step(*inputs, 1)
        runner = GraphedStep(st, inputs, warmup=0, alias_inputs=True) if graph else None
        step = (lambda it: runner.step(inputs, it)) if graph else (lambda it: st.step(*inputs, it))
        step(2)
        eng = next(iter(m._engines.values()))[0]
        assert not eng.last_fwd_packed          # the second forward went without a pack launch
        if write == "load_state_dict":
            m.load_state_dict(_other_weights())
        else:
            p = dict(m.named_parameters())[E.enc_prefix(2) + ".0.weight"]
            p.data.mul_(0.5)
        held = {k: v.detach().clone() for k, v in m.state_dict().items()}
        got = step(3)["logits"].detach().clone()
        torch.cuda.synchronize()
        fresh = UNet(1, 4).to(DEV)
        fresh.load_state_dict(held)
        fresh.train()
        fresh.external_dropout_masks = masks
        want = fresh(torch.cat([inputs[0], inputs[2]], 0)).detach()
        assert _same(got, want)


# ---- schedule -------------------------------------------------------------------------------------------------------------------------
def _forward_tags(m, x):
    """MarkLog tags of one train-mode forward (as tools/record_engine_schedule.py records them; no_grad, so that the engine is free again)."""
    if not m._engines:
        m._acquire_engine(x)      # (creates the engine; its state is set again by the forward)
    eng = next(iter(m._engines.values()))[0]
    log = eng.marks = MarkLog(DEV)
    try:
        with torch.no_grad():
            m(x)
        torch.cuda.synchronize()
    finally:
        eng.marks = None
    return [span[0] for span in log.spans]


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
def test_schedule_drops_the_pack_launch_only_where_fragments_are_current(math):
    reset_dropout_streams()
    torch.manual_seed(7)
    m = UNet(1, 4).to(DEV)
    m.math = math
    m.train()
    st = SupervisedStep(m, opt_args(), None)
    x, y = _inputs()[:2]
    first = _forward_tags(m, x)
    assert "pack_weights" in first[:3], first[:3]      # a fresh model's first forward packs (beside the first conv: forked behind the calibration stamp)
    st.step(x, y, 1)
    tags = _forward_tags(m, x)
    assert any(t.startswith("fwd:") for t in tags)
    assert ("pack_weights" in tags) == (math == "f32"), tags[:4]
