"""Kernel schedule of one U-Net forward / backward pass on the HIP library.

The engine owns the device workspace for a fixed (N, H, W) problem: the raw (pre-BatchNorm) output of every conv, the
per-layer BatchNorm tables, packed weights, gradient buffers.  It issues the C-ABI calls of include/hpfg_hip.h in the
order of the reference graph (model/unet.py:61-117); no tensor op of the network runs in PyTorch.

Layer naming follows the reference's state_dict keys (e.g. ``encoder.down1.maxpool_conv.1.conv_conv.0``).
"""
from __future__ import annotations

import ctypes as C
import itertools
import os
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

from . import _lib as L

SEED_BUMP = -1      # seed_step value: advance the engine's seed word on the device (inside the forward's first launch)

WIDTHS = (16, 32, 64, 128, 256)          # model/unet.py:161
ENC_DROPOUT = (0.05, 0.1, 0.2, 0.3, 0.5)  # model/unet.py:162
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


ACC, LOCAL, ALLREDUCE, PEER, EVAL = "acc", "local", "allreduce", "peer", "eval"


def bn_route(train: bool, math: int, bn_acc_on: bool, peer: bool, world: int, force_sync: bool) -> str:
    """Where the BatchNorm sums of one pass go, from the engine's switches as they stand when it begins.  ACC: the integer accumulators, read by
    the consumers' prologues, ONE finalize launch per pass (bf16x3 kernels, per-rank statistics, no peer context); LOCAL: per-layer partial rows
    + a finalize launch per layer; ALLREDUCE: partial rows -> hpfg_reduce_partials -> the `allreduce` callable -> finalize; PEER: partial rows
    -> the peer-mailbox *_finalize_x kernels; EVAL: no sums (a forward on the running statistics)."""
    if not train:
        return EVAL
    sync = world > 1 or force_sync
    if bn_acc_on and math == L.MATH_BF16X3 and not peer and not sync:
        return ACC
    if sync:
        return PEER if peer else ALLREDUCE
    return LOCAL


def _pad16(c: int) -> int:
    return (c + 15) // 16 * 16


def _carve(flat: torch.Tensor, sizes: Dict[str, int]) -> Dict[str, torch.Tensor]:
    """name -> consecutive views of `flat`, sizes[name] elements each."""
    ends = list(itertools.accumulate(sizes.values()))
    return {name: flat[e - n:e] for (name, n), e in zip(sizes.items(), ends)}


class DescTable:
    """A ctypes descriptor array and its device copy: the multi-layer launches read the device one and validate the host one."""

    def __init__(self, descs: C.Array, dev: torch.device):
        self.host = descs
        self.dev = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
        self._base, self._size = self.dev.data_ptr(), C.sizeof(descs._type_)

    def sub(self, lo: int, hi: int):
        """(device pointer, host view, count) of descriptors [lo, hi); the host view aliases the array."""
        return self._base + lo * self._size, (self.host._type_ * (hi - lo)).from_buffer(self.host, lo * self._size), hi - lo


@dataclass
class ConvSpec:
    name: str            # state_dict prefix of the conv ("….weight", "….bias")
    bn: Optional[str]    # state_dict prefix of its BatchNorm, or None
    cin: int
    cout: int
    taps: int
    h: int               # output height / width
    w: int
    drop_p: float = 0.0  # dropout applied to this layer's activated output
    idx: int = 0
    cin_pad: int = 0
    cout_pad: int = 0

    def __post_init__(self):
        self.cin_pad, self.cout_pad = _pad16(self.cin), _pad16(self.cout)


def enc_prefix(lvl: int) -> str:
    return "encoder.in_conv.conv_conv" if lvl == 0 else f"encoder.down{lvl}.maxpool_conv.1.conv_conv"


def build_specs(in_ch: int, ncls: int, H: int, W: int) -> Dict[str, ConvSpec]:
    specs: Dict[str, ConvSpec] = {}

    def add(s: ConvSpec):
        s.idx = len(specs)
        specs[s.name] = s

    cprev = in_ch
    for lvl, c in enumerate(WIDTHS):
        p, h, w = enc_prefix(lvl), H >> lvl, W >> lvl
        add(ConvSpec(f"{p}.0", f"{p}.1", cprev, c, 9, h, w, ENC_DROPOUT[lvl]))
        add(ConvSpec(f"{p}.4", f"{p}.5", c, c, 9, h, w))
        cprev = c
    for k in range(1, 5):
        c1, c2 = WIDTHS[5 - k], WIDTHS[4 - k]
        hl, wl = H >> (5 - k), W >> (5 - k)
        add(ConvSpec(f"decoder.up{k}.conv1x1", None, c1, c2, 1, hl, wl))
        p = f"decoder.up{k}.conv.conv_conv"
        add(ConvSpec(f"{p}.0", f"{p}.1", 2 * c2, c2, 9, 2 * hl, 2 * wl))
        add(ConvSpec(f"{p}.4", f"{p}.5", c2, c2, 9, 2 * hl, 2 * wl))
    add(ConvSpec("decoder.out_conv", None, WIDTHS[0], ncls, 9, H, W))
    return specs


class MarkLog:
    """Device time stamps around selected launches (bench.py's per-kernel timings).  A stamp is a one-wave kernel that stores s_memrealtime
    (100 MHz) into a slot of `buf` (hpfg_timestamp); stamps are ordinary stream work, so they are captured into a hipGraph with the launches
    they bracket and every replay refreshes them -- no host events, no eager steps.  `spans`: (tag, first slot, last slot) in capture
    order; a ("calib", ...) span brackets nothing: its length (one stamp kernel plus one kernel boundary) is what a bracket costs by itself."""

    def __init__(self, dev: torch.device, capacity: int = 2048):
        self.buf = torch.zeros(capacity, dtype=torch.int64, device=dev)
        self.spans: List[tuple] = []
        self.n = 0
        self.lib = L.load()

    def stamp(self, stream: int) -> int:
        k = self.n
        if k >= self.buf.numel():
            raise RuntimeError("MarkLog: out of slots")
        self.n += 1
        L.check(self.lib.hpfg_timestamp(self.buf.data_ptr() + 8 * k, stream), "timestamp")
        return k

    def bracket(self, tag: str, stream: int, launch):
        a = self.stamp(stream)
        launch()
        self.spans.append((tag, a, self.stamp(stream)))

    def calib(self, stream: int):
        a = self.stamp(stream)
        self.spans.append(("calib", a, self.stamp(stream)))

    def read_us(self) -> List[tuple]:
        """[(tag, microseconds)] of the last execution (synchronises)."""
        t = self.buf[: self.n].cpu().numpy()
        return [(tag, float(int(t[b]) - int(t[a])) / 100.0) for tag, a, b in self.spans]


class UNetEngine:
    """Forward/backward schedule for one (module, N, H, W).  ``params``: name -> tensor views (flat buffers of the module)."""

    def __init__(self, params: Dict[str, torch.Tensor], buffers: Dict[str, torch.Tensor], grads: Dict[str, torch.Tensor],
                 in_ch: int, ncls: int, N: int, H: int, W: int, device: torch.device):
        assert H % 16 == 0 and W % 16 == 0, "U-Net input must be a multiple of 16 (4 poolings)"
        self.lib = L.load()
        self.dev = device
        self.N, self.H, self.W, self.in_ch, self.ncls = N, H, W, in_ch, ncls
        self.params, self.buffers, self.grads = params, buffers, grads
        self.specs = build_specs(in_ch, ncls, H, W)
        self.order = list(self.specs.values())
        f32 = dict(dtype=torch.float32, device=device)
        # raw conv outputs (logits are allocated per forward call)
        self.z: Dict[str, torch.Tensor] = {s.name: torch.empty(N, s.h, s.w, s.cout, **f32) for s in self.order if s.name != "decoder.out_conv"}
        self.bn: Dict[str, torch.Tensor] = {s.name: torch.zeros(L.BN_ROWS, s.cout, **f32) for s in self.order if s.bn}
        nb = max(self.lib.hpfg_conv_stat_blocks(N, s.h, s.w) * 2 * s.cout_pad for s in self.order if s.bn)
        nb = max(nb, max(self.lib.hpfg_bn_bwd_blocks(N, s.h, s.w, s.cout) * 2 * s.cout for s in self.order if s.bn))
        nb = max(nb, max(self.lib.hpfg_bn_bwd_pool_blocks(N, s.h // 2, s.w // 2, s.cout) * 2 * s.cout for s in self.order if s.bn))
        self.partials = torch.empty(nb, **f32)
        self.sums = torch.empty(2 * 256, dtype=torch.float64, device=device)
        # packed weights (the first conv reads OIHW directly)
        self.packed = [s for s in self.order if s.idx > 0]
        self.wpk_f = {s.name: torch.empty(s.taps * s.cin_pad * s.cout_pad, **f32) for s in self.packed}
        self.wpk_d = {s.name: torch.empty(s.taps * s.cin_pad * s.cout_pad, **f32) for s in self.packed}
        self.bias_pad = {s.name: torch.empty(s.cout_pad, **f32) for s in self.packed}
        # bf16x3 fragments (hi/lo split weights) for the split-precision matrix-core path
        self.kc = {s.name: self.lib.hpfg_conv_kc(s.h, s.w, s.taps) for s in self.packed}
        self.wpk16_f = {s.name: torch.empty(self.lib.hpfg_wpk16_elems(s.cin, s.cout_pad, s.taps, self.kc[s.name]), dtype=torch.bfloat16, device=device)
                        for s in self.packed}
        self.wpk16_d = {s.name: torch.empty(self.lib.hpfg_wpk16_elems(s.cout, s.cin_pad, s.taps, self.kc[s.name]), dtype=torch.bfloat16, device=device)
                        for s in self.packed}
        self._pack_tables: Dict[tuple, DescTable] = {}   # (math, with_dgrad) -> descriptors, built on first use
        # Fragments the optimizer's update launch wrote (hpfg_sgd_ema_pack_step, utils/optim.py) are CURRENT: the next forward starts without a
        # pack launch.  frag_token: what the owner's weights looked like to the host when they were written (UNet._weights_token), None = stale;
        # the model compares it in front of every forward and says so in frag_ok.  Anything else that writes weights leaves them stale.
        self.frag_token, self.frag_dgrad, self.frag_ok = None, False, False
        self.pads_zeroed: set = set()      # "f" / "d": a full bf16x3 pack has written that layout once, padding included (the update launch writes weights only)
        self.last_fwd_packed = True
        self._first_bump: Optional[tuple] = None      # (counters, seed_add) for the first conv of a forward that does not pack
        # BatchNorm sums through integer atomics (csrc/common.h: hpfg_acc_add): a conv adds its per-channel sums to the layer's accumulator and
        # every forward consumer derives scale / shift from it in its prologue, so NO finalize launch sits between two convs; ONE launch at the
        # end of the forward (hpfg_bn_acc_finalize) writes all 18 tables for the backward kernels and the running statistics.  bf16x3 kernels,
        # per-rank statistics only (the global-batch data-parallel mode exchanges the sums inside its finalize kernels and keeps them).
        self.bn_layers = [s for s in self.order if s.bn]      # (encoder layers first: build_specs order)
        self._bn_idx = {s.name: i for i, s in enumerate(self.bn_layers)}
        self._n_enc_bn = sum(1 for s in self.bn_layers if s.name.startswith("encoder."))
        self.bn_acc_on = os.environ.get("HPFG_BN_ACC", "1") != "0"      # 0: the per-layer finalize launches (the path the global-batch data-parallel mode keeps)
        # shards: the producers' same-address atomics want many (ONE shard: +0.3 ms per step, two: +0.09), every consumer workgroup's prologue
        # wants few (32 bytes per channel and shard).  Measured in the step (profiles/r04_bn_acc.txt): 8 everywhere beats 4 and beats 8 / 4 / 2 by
        # channel count -- the contention costs more than the prologue reads.
        self.acc_shards = {s.name: L.ACC_MAX_SHARDS for s in self.bn_layers}
        assert all(s.cout == s.cout_pad for s in self.bn_layers)
        acc_words = {s.name: self.acc_shards[s.name] * 4 * s.cout for s in self.bn_layers}
        self.acc_all = torch.zeros(sum(acc_words.values()), dtype=torch.int64, device=device)
        self.acc_of = _carve(self.acc_all, acc_words)
        self.fwd_route, self._acc_dirty = EVAL, False      # bn_route of the last forward (backward and materialize read its virtual inputs again)
        self._acc_tables: Dict[bool, DescTable] = {}      # track_running -> descriptors of hpfg_bn_acc_finalize
        # set by the model for the network that runs on the step's ORIGIN stream (the single trainable network of a step): its weight packing
        # (22 us) runs on the side stream beside the first conv, which reads the OIHW weights directly and needs nothing the launch produces
        self.pack_overlap = False
        self.after_layer = None      # (layer index, callable): the step enqueues another network's forward behind that layer (graph submission order)
        # the same for the backward sums (sum g, sum g * xhat): added by the dgrad epilogue / the reduction pass that completes a layer's
        # gradient, read by every dZ consumer's prologue (k1 .. k3 derived there), turned into dgamma / dbeta -- and zeroed again -- by ONE
        # launch per backward (hpfg_bn_acc_bwd_finalize) instead of 18 finalize launches on the critical chain
        self.accb_all = torch.zeros_like(self.acc_all)
        self.accb_of = _carve(self.accb_all, acc_words)
        self.bwd_route, self._accb_dirty = LOCAL, False      # bn_route of the backward pass in progress
        self._accb_table: Optional[DescTable] = None
        self.seed_dev = torch.zeros(1, dtype=torch.int32, device=device)   # run-time dropout seed word
        self.bump_counters: Optional[torch.Tensor] = None      # set by the module in front of a train-mode forward: int64 counters the pack launch advances
        self.base_seed = 0x1234567
        self.dropout_on = False      # does the forward in progress / last forward draw dropout masks (its backward applies the same ones)
        self._stage_inputs = False      # act_side of this forward: the convs below the aligned levels store the input they stage
        self.bwd_ready = False
        self.x: Optional[torch.Tensor] = None
        self.world = 1
        self.gtmp, self.direct = None, False      # set by the model: the buffer `grads` views; direct: it IS the flat gradient buffer (no staging copy)
        # backward workspace, filled by _alloc_bwd on the first backward: gradients w.r.t. activations (dA: of each BatchNorm'd conv's output;
        # dcat / dup: the decoder's concatenations; dU: the 1x1 convs' outputs; dP: the max-pools' outputs), weight-gradient slabs, bias-gradient rows
        self._bwd_alloc_key: Optional[tuple] = None      # what the layout was built for; None: not built yet
        self.dA, self.dA_ps = {}, {}      # layer -> tensor, pixel stride
        self.dcat, self.dup, self.dU, self.dP = {}, {}, {}, {}      # decoder block / encoder level -> tensor
        self.slab_of, self.csum_part, self.csum_rows = {}, {}, {}      # layer -> slab region; bias-gradient rows and their count
        self.slabs: Optional[DescTable] = None
        self.bias_layers = [s for s in self.order if not s.bn]
        # slab descriptor order = encoder convs | decoder convs | bias pseudo layers (all decoder): two contiguous ranges, so the decoder's
        # weight gradients can be finished (and handed to the data-parallel all-reduce) while the encoder half still back-propagates
        self._n_enc_desc = sum(1 for s in self.order if s.name.startswith("encoder."))
        # encoder levels 0 and 1 (in_conv, down1) come first: their slabs are written last (by the main stream's final kernels)
        self._n_thin_enc_desc = sum(1 for s in self.order if s.name.startswith("encoder.in_conv") or s.name.startswith("encoder.down1"))
        # BatchNorm-backward sums of the layer below from the dgrad epilogue (bf16x3 kernels) instead of a streaming pass of their own
        self.fuse_bwd_stats = 1      # 0: a streaming pass per layer (tests); 2: also the register-starved 32-channel instantiation
        self._fused_rows: Dict[str, int] = {}
        # thin 3x3 layers (16-pixel-aligned, <= 64 input / 32 output channels, split-bf16 math): ONE kernel produces the input gradient, the
        # weight-gradient slabs and the backward sums of the layer below from a single staging of dZ (hpfg_fused_bwd)
        self.fused_bwd = os.environ.get("HPFG_FUSED_BWD", "1") == "1"
        # HpfgConvArgs.stage_out: the separate dgrad of a 3x3 layer also stores the dZ it stages, and (act_side) its forward conv the virtual
        # input it stages; the layer's weight gradient reads those tensors as PLAIN sources instead of deriving both again -- BatchNorm,
        # LeakyReLU, Dropout, max-pool / bilinear taps forward, their backward for dZ -- in every (input slice x output slice) workgroup
        # the max-pool backward + BatchNorm-backward sums of a block output ride in the epilogue of the dgrad that produces dP (56 / 28 / 14-pixel levels)
        self.pool_fuse = True
        self._pool_done: set = set()
        self.dz_side = True      # (attributes, not environment switches: tests and A/B tools set them on the engine)
        self.act_side = True
        # the upsample backward of a decoder block is gathered by the 1x1 conv's dgrad while it stages its tiles (HPFG_ACT_UPBWD) instead of
        # by a launch of its own in front of it
        self.upb_fuse = os.environ.get("HPFG_UPB_FUSE", "1") == "1"
        self.upb_max_c1 = int(os.environ.get("HPFG_UPB_MAX_C1", "128"))
        self.dzbuf: Dict[str, torch.Tensor] = {}
        self.actbuf: Dict[str, torch.Tensor] = {}
        self._act_live: set = set()      # layers whose actbuf this forward wrote
        # set by the model (UNet.defer_wgrad, which the single-network step objects switch on).  Not with two trainable networks
        # back-propagating on two streams: the fork below would then leave a FORKED stream, and an event wait between two non-origin
        # streams of a capture makes hipStreamEndCapture fault on ROCm 7.2 (tools/nested_fork_probe.py reproduces it without this code)
        self.defer_wgrad = False
        self._deferred: Optional[list] = None      # (layer, dZ source) of the weight gradients queued for the side stream; None: not deferring
        self._csum_pending: Optional[torch.Tensor] = None      # dlogits while out_conv's bias sums wait for the first queued batch
        self.fused_grid: Dict[str, int] = {}      # layer -> workgroups (= slabs) of its hpfg_fused_bwd launch, fixed by _alloc_bwd
        self._side, self._side_used = None, False      # side stream (_fork_side creates it); backward queued work there that is not joined yet
        self.force_sync = False  # run the data-parallel code path (reduce -> all-reduce -> finalize) even with one rank (tests)
        self.math = L.MATH_F32      # L.MATH_BF16X3 selects the split-bf16 matrix-core kernels for conv forward / dgrad
        self.ext_masks: Dict[str, torch.Tensor] = {}   # conv name -> uint8 NHWC keep-mask (parity tests replaying torch's masks)
        self.allreduce = None    # callable(tensor) -> in-place sum across ranks (data parallel), set by hpfg_amd.parallel
        # peer mailbox exchange (hpfg_amd.parallel.DataParallelContext.enable_peer_exchange): the finalize kernels add the ranks' sums
        # themselves -- no collective between the kernels.  peer = the context, peer_base = first of this engine's 2 x 18 mailbox slots,
        # xepoch = device word counting this engine's train-mode forwards (the epoch of every slot use of that forward / its backward)
        self.peer, self.peer_base, self.xepoch = None, 0, None
        self.marks: Optional[MarkLog] = None      # bench.py: device time stamps around every conv / dgrad / wgrad / BatchNorm launch

    # ---------------------------------------------------------------------------------------------------------
    def _stream(self):
        return torch.cuda.current_stream(self.dev).cuda_stream

    def _call(self, fn, *args, tag: Optional[str] = None, stream: Optional[int] = None):
        """fn(*args, stream) of the library, its status checked -- bracketed by device time stamps on that stream when the launch has a tag and a
        MarkLog is attached.  A failure names the entry point and, through the tag, the pass and the layer."""
        st = self._stream() if stream is None else stream

        def launch():
            L.check(fn(*args, st), f"{fn.__name__}[{tag}]" if tag else fn.__name__)
        if tag is None or self.marks is None:
            return launch()
        self.marks.bracket(tag, st, launch)

    @property
    def _b16(self) -> bool:
        return self.math == L.MATH_BF16X3

    def _fork_side(self) -> torch.cuda.Stream:
        """The side stream, ordered behind everything queued on the current stream so far."""
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.dev)
        self._side.wait_stream(torch.cuda.current_stream(self.dev))
        return self._side

    def _join_side(self):
        if self._side_used:
            torch.cuda.current_stream(self.dev).wait_stream(self._side)
            self._side_used = False

    def layer_seed(self, s: ConvSpec) -> int:
        return (self.base_seed * 0x9E3779B1 + 0x85EBCA6B * (s.idx + 1)) & 0xFFFFFFFF

    def _act_bn(self, name: str, mode=L.ACT_BNACT) -> L.Act:
        s = self.specs[name]
        a = L.Act()
        a.z, a.bn, a.mode, a.C = L.ptr(self.z[name]), L.ptr(self.bn[name]), mode, s.cout
        a.Hs, a.Ws, a.pstride, a.bn_stride, a.bn_coff = s.h, s.w, s.cout, s.cout, 0
        if self.fwd_route == ACC and mode in (L.ACT_BNACT, L.ACT_BNACT_POOL):      # the forward consumers form scale / shift from the sums themselves
            a.bn_acc, a.bn_gamma, a.bn_beta = L.ptr(self.acc_of[name]), L.ptr(self.params[f"{s.bn}.weight"]), L.ptr(self.params[f"{s.bn}.bias"])
            a.bn_count, a.bn_eps, a.bn_shards = float(self.N * s.h * s.w), BN_EPS, self.acc_shards[name]
        if mode == L.ACT_BNACT:
            self._act_dropout(a, s)
        return a

    def _act_dropout(self, a: L.Act, s: ConvSpec):
        if s.drop_p > 0 and self.dropout_on:
            a.drop_p, a.drop_seed, a.seed_dev = s.drop_p, self.layer_seed(s), L.ptr(self.seed_dev)
            a.drop_mask = L.ptr(self.ext_masks.get(s.name)) if self.ext_masks else None

    def _act_plain(self, t: torch.Tensor, C_: int, h: int, w: int, pstride: Optional[int] = None, mode=L.ACT_PLAIN) -> L.Act:
        a = L.Act()
        a.z, a.mode, a.C, a.Hs, a.Ws = L.ptr(t), mode, C_, h, w
        a.pstride = C_ if pstride is None else pstride
        if C_ % 4 != 0 and mode == L.ACT_PLAIN:
            a.mode = L.ACT_STRIDED
            a.sn, a.sc, a.sy, a.sx = h * w * a.pstride, 1, w * a.pstride, a.pstride
        return a

    def _act_split(self, t: torch.Tensor, C_: int, h: int, w: int) -> L.Act:
        """A side tensor stored by HpfgConvArgs.stage_out: bf16 [N][h][w][C / 8][hi 8 | lo 8] in a buffer of N*h*w*C fp32 words."""
        return self._act_plain(t, C_, h, w, mode=L.ACT_SPLIT16)

    def _act_input(self, x: torch.Tensor) -> L.Act:
        a = L.Act()
        a.z, a.mode, a.C, a.Hs, a.Ws = L.ptr(x), L.ACT_STRIDED, self.in_ch, self.H, self.W
        a.sn, a.sc, a.sy, a.sx = x.stride(0), x.stride(1), x.stride(2), x.stride(3)
        return a

    def _act_dz(self, name: str, dA: torch.Tensor, da_pstride: int) -> L.Act:
        s = self.specs[name]
        a = L.Act()
        a.z, a.bn, a.aux, a.mode, a.C = L.ptr(self.z[name]), L.ptr(self.bn[name]), L.ptr(dA), L.ACT_DZ, s.cout
        a.Hs, a.Ws, a.pstride, a.aux_pstride, a.bn_stride = s.h, s.w, s.cout, da_pstride, s.cout
        if self.bwd_route == ACC:          # the dZ consumers form k1 .. k3 from the backward sums themselves
            a.bn_acc, a.bn_gamma, a.bn_count, a.bn_shards = L.ptr(self.accb_of[name]), L.ptr(self.params[f"{s.bn}.weight"]), float(self.N * s.h * s.w), self.acc_shards[name]
        self._act_dropout(a, s)
        return a

    def input_acts(self, name: str):
        """(a0, a1) virtual input of conv `name` (forward view)."""
        s = self.specs[name]
        none = L.Act()
        if name == "encoder.in_conv.conv_conv.0":
            return self._act_input(self.x), none
        if name == "decoder.out_conv":
            return self._act_bn("decoder.up4.conv.conv_conv.4"), none
        if name.endswith(".4"):
            return self._act_bn(name[:-2] + ".0"), none
        if name.startswith("encoder.down"):
            lvl = int(name[len("encoder.down")])
            return self._act_bn(enc_prefix(lvl - 1) + ".4", L.ACT_BNACT_POOL), none
        k = int(name[len("decoder.up")])
        prev = enc_prefix(4) + ".4" if k == 1 else f"decoder.up{k - 1}.conv.conv_conv.4"
        if name.endswith("conv1x1"):
            return self._act_bn(prev), none
        # decoder block conv 0: cat([skip, up(conv1x1)])
        skip = self._act_bn(enc_prefix(4 - k) + ".4")
        u = self.specs[f"decoder.up{k}.conv1x1"]
        up = self._act_plain(self.z[u.name], u.cout, u.h, u.w, mode=L.ACT_UP2X)
        return skip, up

    # ---------------------------------------------------------------------------------------------------------
    def _pack_table(self, math: int, with_dgrad: bool):
        """Descriptor table for hpfg_pack_weights: only the fragment layouts this math mode / pass consumes are produced (the
        fp32 fragments in exact-fp32 mode, the split-bf16 ones in bf16x3 mode; the dgrad transposes only if a backward follows)."""
        key = (math, with_dgrad)
        if key not in self._pack_tables:
            b16 = math == L.MATH_BF16X3
            descs = (L.PackDesc * len(self.packed))()
            for d, s in zip(descs, self.packed):
                d.w_oihw, d.b = L.ptr(self.params[f"{s.name}.weight"]), L.ptr(self.params[f"{s.name}.bias"])
                d.bias_pad = L.ptr(self.bias_pad[s.name])
                d.wpk_fwd = None if b16 else L.ptr(self.wpk_f[s.name])
                d.wpk_dgrad = None if (b16 or not with_dgrad) else L.ptr(self.wpk_d[s.name])
                d.wpk16_fwd = L.ptr(self.wpk16_f[s.name]) if b16 else None
                d.wpk16_dgrad = L.ptr(self.wpk16_d[s.name]) if (b16 and with_dgrad) else None
                d.kc = self.kc[s.name]
                d.Cout, d.Cin, d.CoutPad, d.CinPad, d.taps = s.cout, s.cin, s.cout_pad, s.cin_pad, s.taps
            self._pack_tables[key] = DescTable(descs, self.dev)
        return self._pack_tables[key]

    def pack(self, with_dgrad: bool = True, counters: Optional[torch.Tensor] = None, seed_add: int = 0):
        """counters: int64 tensor whose elements the same launch advances by one (num_batches_tracked of the network's BatchNorm layers);
        seed_add: advance of the engine's dropout seed word (hpfg_pack_weights_bump)."""
        dev, host, n = self._pack_table(self.math, with_dgrad).sub(0, len(self.packed))
        if counters is not None:
            assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.device == self.dev
        self._call(self.lib.hpfg_pack_weights_bump, dev, host, n, L.ptr(counters), counters.numel() if counters is not None else 0, L.ptr(self.seed_dev), int(seed_add),
                   None, 0, tag="pack_weights")
        if self._b16:
            self.pads_zeroed |= {"f", "d"} if with_dgrad else {"f"}

    def _finalize_bwd_all(self, lo: int, hi: int):
        """hpfg_bn_acc_bwd_finalize for BatchNorm layers [lo, hi) of self.bn_layers (encoder layers come first): dgamma / dbeta (+ the k rows)
        from the backward accumulators, which the launch zeroes again."""
        if self.bwd_route != ACC or hi <= lo:
            return
        if self._accb_table is None:
            descs = (L.BnAccBwdDesc * len(self.bn_layers))()
            for d, s in zip(descs, self.bn_layers):
                d.acc, d.gamma, d.bn = L.ptr(self.accb_of[s.name]), L.ptr(self.params[f"{s.bn}.weight"]), L.ptr(self.bn[s.name])
                d.dgamma, d.dbeta = L.ptr(self.grads[f"{s.bn}.weight"]), L.ptr(self.grads[f"{s.bn}.bias"])
                d.C, d.count, d.shards = s.cout, float(self.N * s.h * s.w), self.acc_shards[s.name]
            self._accb_table = DescTable(descs, self.dev)
        dev, host, n = self._accb_table.sub(lo, hi)
        self._call(self.lib.hpfg_bn_acc_bwd_finalize, dev, host, n, tag="bn_bfin_all")

    def _finalize_all(self, track: bool):
        """hpfg_bn_acc_finalize: every BatchNorm table of this forward (+ running statistics) in one launch, from the sum accumulators."""
        if track not in self._acc_tables:
            descs = (L.BnAccDesc * len(self.bn_layers))()
            for d, s in zip(descs, self.bn_layers):
                d.acc, d.gamma, d.beta = L.ptr(self.acc_of[s.name]), L.ptr(self.params[f"{s.bn}.weight"]), L.ptr(self.params[f"{s.bn}.bias"])
                d.running_mean = L.ptr(self.buffers[f"{s.bn}.running_mean"]) if track else None
                d.running_var = L.ptr(self.buffers[f"{s.bn}.running_var"]) if track else None
                d.bn, d.C, d.count, d.shards = L.ptr(self.bn[s.name]), s.cout, float(self.N * s.h * s.w), self.acc_shards[s.name]
            self._acc_tables[track] = DescTable(descs, self.dev)
        dev, host, n = self._acc_tables[track].sub(0, len(self.bn_layers))
        self._call(self.lib.hpfg_bn_acc_finalize, dev, host, n, BN_MOMENTUM, BN_EPS, tag="bn_fin_all")

    def _finalize_bn(self, s: ConvSpec, nblk: int, track: bool):
        """BatchNorm table (+ running statistics) of layer s from the nblk partial rows its conv left (every route but ACC)."""
        rm, rv = (L.ptr(self.buffers[f"{s.bn}.running_{k}"]) if track else None for k in ("mean", "var"))
        # (count, gamma, beta, running mean / variance, momentum, eps, table, C): the same for every route
        tail = (float(self.N * s.h * s.w * self.world), L.ptr(self.params[f"{s.bn}.weight"]), L.ptr(self.params[f"{s.bn}.bias"]), rm, rv,
                BN_MOMENTUM, BN_EPS, L.ptr(self.bn[s.name]), s.cout)
        if self.fwd_route == PEER:
            px = self.peer.peer_desc(self.peer_base + 2 * self._bn_idx[s.name], self.xepoch)
            self._call(self.lib.hpfg_bn_fwd_finalize_x, L.ptr(self.partials), nblk, C.byref(px), *tail, tag="bn_fin:" + s.name)
        elif self.fwd_route == ALLREDUCE:
            sums = self.sums[: 2 * s.cout_pad]
            self._call(self.lib.hpfg_reduce_partials, L.ptr(self.partials), nblk, s.cout_pad, L.ptr(sums))
            self.allreduce(sums)
            self._call(self.lib.hpfg_bn_fwd_finalize, None, 0, L.ptr(sums), *tail)
        else:
            self._call(self.lib.hpfg_bn_fwd_finalize, L.ptr(self.partials), nblk, None, *tail, tag="bn_fin:" + s.name)

    def forward(self, x: torch.Tensor, train: bool = True, dropout: Optional[bool] = None, track_running: bool = True,
                seed_step: Optional[int] = None, needs_grad: bool = True) -> torch.Tensor:
        """x: [N,C,H,W] fp32 on the device (any strides).  Returns logits as an [N,H,W,ncls] tensor (fresh allocation)."""
        pack_args = self._fwd_begin(x, train, dropout, seed_step, needs_grad)
        logits = torch.empty(self.N, self.H, self.W, self.ncls, dtype=torch.float32, device=self.dev)
        for i, s in enumerate(self.order):
            if i == 0 and pack_args is not None:
                # one fork / join against the stream this forward runs on (the step's origin stream: UNet sets pack_overlap only there -- a fork
                # of a forked stream inside a capture faults in hipStreamEndCapture on ROCm 7.2): [pack] beside [first conv]
                main = torch.cuda.current_stream(self.dev)
                with torch.cuda.stream(self._fork_side()):
                    self.pack(**pack_args)
                self._fwd_layer(s, logits, track_running)
                main.wait_stream(self._side)
                continue
            self._fwd_layer(s, logits, track_running)
            if self.after_layer is not None and i == self.after_layer[0]:
                self.after_layer[1]()
        if self.fwd_route == ACC:
            self._finalize_all(track_running)
            self._acc_dirty = False
        self.bwd_ready = bool(train and needs_grad)
        return logits

    def _fwd_begin(self, x: torch.Tensor, train: bool, dropout: Optional[bool], seed_step: Optional[int], needs_grad: bool) -> Optional[dict]:
        """Per-forward state and route; the weight packing, unless it is to overlap the first conv: then its arguments are returned."""
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (self.N, self.in_ch, self.H, self.W), (x.shape, x.dtype, x.device)
        self.x = x
        self._act_live = set()
        self._stage_inputs = bool(train and needs_grad and self.act_side and self._b16)
        self.dropout_on = train if dropout is None else dropout
        # seed_step: None = leave the seed word alone; SEED_BUMP = advance it on the device (a step being captured into a hipGraph: every
        # replay then draws new masks); otherwise the host's per-forward counter value
        if seed_step is not None and seed_step != SEED_BUMP:
            self.seed_dev.fill_(int(seed_step) & 0x7FFFFFFF)
        counters, self.bump_counters = self.bump_counters, None
        self.fwd_route = bn_route(train, self.math, self.bn_acc_on, self.peer is not None, self.world, self.force_sync)
        if self.fwd_route == ACC:
            if self._acc_dirty:          # a forward that never reached its finalize launch (an exception): start from zero (hpfg_bn_acc_finalize zeroes otherwise)
                self.acc_all.zero_()
            self._acc_dirty = True
        pack_args = dict(with_dgrad=bool(train and needs_grad), counters=counters, seed_add=1 if seed_step == SEED_BUMP else 0)
        self._first_bump = None
        self.last_fwd_packed = not (self._b16 and self.frag_ok and self.frag_token is not None and (self.frag_dgrad or not pack_args["with_dgrad"]))
        self.frag_ok = False
        if not self.last_fwd_packed:      # current fragments: no pack launch (and no fork for it); the two counters ride in the first conv
            if counters is not None or pack_args["seed_add"]:
                self._first_bump = (counters, pack_args["seed_add"])
            pack_args = None
        elif not (self.pack_overlap and train):
            self.pack(**pack_args)
            pack_args = None
        if self.marks is not None:
            self.marks.calib(self._stream())
        if self.fwd_route == PEER:
            self.peer.bump(self.xepoch, self._stream())      # the epoch of this forward's (and its backward's) mailbox exchanges
        return pack_args

    def _fwd_layer(self, s: ConvSpec, logits: torch.Tensor, track_running: bool):
        """One conv of the schedule (+ its BatchNorm table) on the current stream."""
        out = logits if s.name == "decoder.out_conv" else self.z[s.name]
        want_stats = bool(s.bn) and self.fwd_route != EVAL
        acc = want_stats and self.fwd_route == ACC      # the sums go into the layer accumulator; the consumers (and _finalize_all) take them from there
        if s.idx == 0:
            a0, _ = self.input_acts(s.name)
            w, b = L.ptr(self.params[f"{s.name}.weight"]), L.ptr(self.params[f"{s.name}.bias"])
            if self._first_bump is not None:
                (cnt, seed_add), self._first_bump = self._first_bump, None
                self._call(self.lib.hpfg_conv3x3_first_fwd_bump, C.byref(a0), w, b, L.ptr(out), None if acc or not want_stats else L.ptr(self.partials),
                           L.ptr(self.acc_of[s.name]) if acc else None, self.acc_shards[s.name], L.ptr(cnt), cnt.numel() if cnt is not None else 0,
                           L.ptr(self.seed_dev), int(seed_add), self.N, s.h, s.w, s.cin, s.cout, tag="fwd:" + s.name)
            elif acc:
                self._call(self.lib.hpfg_conv3x3_first_fwd_acc, C.byref(a0), w, b, L.ptr(out), None, L.ptr(self.acc_of[s.name]), self.acc_shards[s.name],
                           self.N, s.h, s.w, s.cin, s.cout, tag="fwd:" + s.name)
            else:
                self._call(self.lib.hpfg_conv3x3_first_fwd, C.byref(a0), w, b, L.ptr(out), L.ptr(self.partials) if want_stats else None,
                           self.N, s.h, s.w, s.cin, s.cout, tag="fwd:" + s.name)
            nblk = self.lib.hpfg_conv_first_rows(self.N, s.h, s.w)
        else:
            ca = L.ConvArgs()
            ca.a0, ca.a1 = self.input_acts(s.name)
            ca.math = self.math
            ca.wpk = L.ptr(self.wpk16_f[s.name]) if self._b16 else L.ptr(self.wpk_f[s.name])
            ca.bias, ca.out = L.ptr(self.bias_pad[s.name]), L.ptr(out)
            ca.out_pstride, ca.Cout, ca.CoutPad = s.cout, s.cout, s.cout_pad
            ca.N, ca.H, ca.W, ca.taps = self.N, s.h, s.w, s.taps
            if acc:
                ca.stat_acc, ca.stat_shards = L.ptr(self.acc_of[s.name]), self.acc_shards[s.name]
            elif want_stats:
                ca.stat_partials = L.ptr(self.partials)
            if self._stage_inputs and self._side_layer(s) and s.cin % 8 == 0 and ca.a0.mode != L.ACT_PLAIN:
                ca.stage_out = L.ptr(self._side_buf(self.actbuf, s, s.cin))
                self._act_live.add(s.name)
            self._call(self.lib.hpfg_conv_fwd, C.byref(ca), tag="fwd:" + s.name)
            if want_stats and not acc:
                nblk = self.lib.hpfg_conv_stat_rows(C.byref(ca))
        if s.bn:
            if self.fwd_route == EVAL:
                self._call(self.lib.hpfg_bn_eval_table, L.ptr(self.params[f"{s.bn}.weight"]), L.ptr(self.params[f"{s.bn}.bias"]), L.ptr(self.buffers[f"{s.bn}.running_mean"]),
                           L.ptr(self.buffers[f"{s.bn}.running_var"]), BN_EPS, L.ptr(self.bn[s.name]), s.cout)
            elif self.fwd_route != ACC:
                self._finalize_bn(s, nblk, track_running)

    def materialize(self, name: str, mode=L.ACT_BNACT) -> torch.Tensor:
        """Activated output of conv `name` as a real [N,h,w,C] tensor (projection-neck input, tests)."""
        s = self.specs[name]
        a = self._act_bn(name, mode)
        h, w = (s.h // 2, s.w // 2) if mode == L.ACT_BNACT_POOL else (s.h, s.w)
        out = torch.empty(self.N, h, w, s.cout, dtype=torch.float32, device=self.dev)
        self._call(self.lib.hpfg_act_materialize, C.byref(a), None, self.N, h, w, L.ptr(out))
        return out

    def materialize_input(self, name: str) -> torch.Tensor:
        """Virtual input of conv `name` ([N,h,w,Cin]) -- what the conv kernel stages into LDS."""
        s = self.specs[name]
        a0, a1 = self.input_acts(name)
        out = torch.empty(self.N, s.h, s.w, s.cin, dtype=torch.float32, device=self.dev)
        self._call(self.lib.hpfg_act_materialize, C.byref(a0), C.byref(a1), self.N, s.h, s.w, L.ptr(out))
        return out

    # ---------------------------------------------------------------------------------------------------------
    def _alloc_bwd(self):
        key = (self.math, self.fused_bwd, self.upb_fuse)      # what the slab layout depends on
        if self._bwd_alloc_key == key:
            return
        self._bwd_alloc_key = key
        f32 = dict(dtype=torch.float32, device=self.dev)
        N, sp = self.N, self.specs
        # gradient w.r.t. each BN'd conv's activated output.  Skip features alias the first half of the decoder's dCat.
        self.dA, self.dA_ps, self.dcat, self.dup = {}, {}, {}, {}
        for k in range(1, 5):
            s = sp[f"decoder.up{k}.conv.conv_conv.0"]
            skip = enc_prefix(4 - k) + ".4"
            # a half of the concat gradient is less than a 128-byte line per pixel (up4: 16 channels): interleaved, every reader of one half
            # would fetch both -> two buffers (HpfgConvArgs.out2).  Otherwise one: dSkip = channels [0, C2) with pixel stride 2*C2
            cw = s.cin // 2 if s.cin // 2 * 4 < 128 else s.cin
            self.dcat[k] = torch.empty(N, s.h, s.w, cw, **f32)
            if cw < s.cin:
                self.dup[k] = torch.empty(N, s.h, s.w, cw, **f32)
            self.dA[skip], self.dA_ps[skip] = self.dcat[k], cw
        for s in self.order:
            if s.bn and s.name not in self.dA:
                self.dA[s.name] = torch.empty(N, s.h, s.w, s.cout, **f32)
                self.dA_ps[s.name] = s.cout
        self.dU = {k: torch.empty(N, s.h, s.w, s.cout, **f32) for k, s in ((k, sp[f"decoder.up{k}.conv1x1"]) for k in range(1, 5))}
        self.dP = {lvl: torch.empty(N, s.h, s.w, s.cin, **f32) for lvl, s in ((lvl, sp[enc_prefix(lvl) + ".0"]) for lvl in range(1, 5))}
        # one slab region per layer; all of them are summed by ONE launch at the end of backward()
        sizes = {s.name: self.lib.hpfg_wgrad_slab_floats(N, s.h, s.w, s.cin_pad, s.cout_pad, s.taps) for s in self.order}
        self.fused_grid = {}
        if self.fused_bwd and self._b16:
            for s in self.order:
                if s.taps != 9:
                    continue
                fa = L.FusedBwdArgs()
                fa.xa0, fa.xa1 = self.input_acts(s.name)
                fa.d.a0.mode = L.ACT_DZ if s.bn else L.ACT_PLAIN
                fa.d.out = None if s.idx == 0 else L.ptr(self.partials)      # (no dX for the first layer: weight gradient only; any non-null otherwise)
                fa.d.N, fa.d.H, fa.d.W, fa.d.taps, fa.d.math = N, s.h, s.w, 9, self.math
                fa.Cin, fa.CinPad, fa.Cout, fa.CoutPad = s.cin, s.cin_pad, s.cout, s.cout_pad
                grid = self.lib.hpfg_fused_bwd_grid(C.byref(fa))
                if grid > 0:
                    self.fused_grid[s.name] = grid
                    sizes[s.name] = max(sizes[s.name], grid * 9 * s.cin_pad * s.cout_pad)
        self.slab_all = torch.empty(sum(sizes.values()), **f32)
        self.slab_of = _carve(self.slab_all, sizes)
        # bias gradients of the convs without BatchNorm (1x1 convs, out_conv): their per-block channel sums are summed by the same
        # launch, as pseudo layers {taps 1, Cin 1} (one kernel less per bias)
        self.csum_rows = {s.name: ((self._upb_rows(s) if self._upb_on(s) else self.lib.hpfg_upsample2x_bwd_blocks(N, s.h, s.w, s.cout)) if s.taps == 1
                                   else self.lib.hpfg_channel_sum_blocks(N * s.h * s.w, s.cout)) for s in self.bias_layers}
        self.csum_part = {s.name: torch.empty(self.csum_rows[s.name] * s.cout, **f32) for s in self.bias_layers}
        descs = (L.SlabDesc * (len(self.order) + len(self.bias_layers)))()
        for d, s in zip(descs, self.order):
            d.slab, d.dw_oihw = L.ptr(self.slab_of[s.name]), L.ptr(self.grads[f"{s.name}.weight"])
            d.S = self.fused_grid.get(s.name) or self.lib.hpfg_wgrad_splits(N, s.h, s.w, s.cin_pad, s.cout_pad, s.taps)
            d.taps, d.Cin, d.CinPad, d.Cout, d.CoutPad = s.taps, s.cin, s.cin_pad, s.cout, s.cout_pad
        for j, s in enumerate(self.bias_layers):
            d = descs[len(self.order) + j]
            d.slab, d.dw_oihw = L.ptr(self.csum_part[s.name]), L.ptr(self.grads[f"{s.name}.bias"])
            d.S = self.csum_rows[s.name]
            d.taps, d.Cin, d.CinPad, d.Cout, d.CoutPad = 1, 1, 1, s.cout, s.cout
        self.slabs = DescTable(descs, self.dev)

    def _bn_backward(self, s: ConvSpec, pooled_grad: Optional[torch.Tensor] = None):
        """BatchNorm/LeakyReLU/Dropout backward statistics of layer s -> k1,k2,k3 rows + dgamma/dbeta.
        pooled_grad: gradient w.r.t. MaxPool2d(2)(this layer's activation) [N,h/2,w/2,C]; it is scattered into dA by the same pass."""
        g = self._act_dz(s.name, self.dA[s.name], self.dA_ps[s.name])
        nblk = self._fused_rows.pop(s.name, None)      # rows the dgrad epilogue that produced dA left (in self.partials / the accumulator)
        if nblk is not None:
            assert pooled_grad is None
        elif self.bwd_route == ACC:
            acc, sh = L.ptr(self.accb_of[s.name]), self.acc_shards[s.name]
            if pooled_grad is not None:
                self._call(self.lib.hpfg_bn_bwd_reduce_pool_acc, C.byref(g), L.ptr(pooled_grad), s.cout, self.N, s.h // 2, s.w // 2, acc, sh, tag="bn_red:" + s.name)
            else:
                self._call(self.lib.hpfg_bn_bwd_reduce_acc, C.byref(g), self.N, s.h, s.w, acc, sh, tag="bn_red:" + s.name)
        elif pooled_grad is not None:
            nblk = self.lib.hpfg_bn_bwd_pool_blocks(self.N, s.h // 2, s.w // 2, s.cout)
            self._call(self.lib.hpfg_bn_bwd_reduce_pool, C.byref(g), L.ptr(pooled_grad), s.cout, self.N, s.h // 2, s.w // 2, L.ptr(self.partials), tag="bn_red:" + s.name)
        else:
            nblk = self.lib.hpfg_bn_bwd_blocks(self.N, s.h, s.w, s.cout)
            self._call(self.lib.hpfg_bn_bwd_reduce, C.byref(g), self.N, s.h, s.w, L.ptr(self.partials), tag="bn_red:" + s.name)
        if self.bwd_route == ACC:      # no finalize launch: the consumers of `g` derive k1 .. k3 from the layer's backward accumulator
            return g
        # (count, gamma, table, dgamma, dbeta, C): the same for every route
        tail = (float(self.N * s.h * s.w * self.world), L.ptr(self.params[f"{s.bn}.weight"]), L.ptr(self.bn[s.name]), L.ptr(self.grads[f"{s.bn}.weight"]),
                L.ptr(self.grads[f"{s.bn}.bias"]), s.cout)
        if self.bwd_route == PEER:
            px = self.peer.peer_desc(self.peer_base + 2 * self._bn_idx[s.name] + 1, self.xepoch)
            self._call(self.lib.hpfg_bn_bwd_finalize_x, L.ptr(self.partials), nblk, C.byref(px), *tail, 1.0 / self.world, tag="bn_bfin:" + s.name)
        elif self.bwd_route == ALLREDUCE:
            sums = self.sums[: 2 * s.cout]
            self._call(self.lib.hpfg_reduce_partials, L.ptr(self.partials), nblk, s.cout, L.ptr(sums))
            self.allreduce(sums)
            self._call(self.lib.hpfg_bn_bwd_finalize, None, 0, L.ptr(sums), *tail, 1.0 / self.world)      # global sums on every rank: the SUM all-reduce of the gradients restores them
        else:
            self._call(self.lib.hpfg_bn_bwd_finalize, L.ptr(self.partials), nblk, None, *tail, 1.0, tag="bn_bfin:" + s.name)
        return g

    def _wgrad_dgrad(self, s: ConvSpec, g: L.Act, dgrad_out: torch.Tensor, stats_for: Optional[str] = None, out2: Optional[torch.Tensor] = None,
                     pool_of: Optional[str] = None):
        """Both gradients of layer s from the same dZ source (they only read it, so their order is free)."""
        if s.name in self.fused_grid:
            return self._fused_bwd(s, g, dgrad_out, stats_for, out2)      # (pool_of: the fused kernel's variant measured mixed, profiles/r04_schedule_experiments.txt)
        dz, gw = None, g      # gw: the weight gradient's dZ source -- the tensor the dgrad stores while it stages, where it does
        if self.dz_side and self._b16 and self._side_layer(s) and g.mode == L.ACT_DZ and s.cout % 8 == 0:
            dz = self._side_buf(self.dzbuf, s, s.cout)
            gw = self._act_split(dz, s.cout, s.h, s.w)
        if self._deferred is None and dz is None:
            self._wgrad(s, g)
        self._dgrad(s, g, dgrad_out, stats_for, out2, stage_out=dz, pool_of=pool_of)
        if self._deferred is not None:      # decoder half: the weight gradient is queued for the side stream (see backward())
            self._deferred.append((s, gw))
        elif dz is not None:
            self._wgrad(s, gw)

    def _upb_on(self, su: ConvSpec) -> bool:
        """Does the dgrad of this decoder 1x1 conv gather the upsample backward itself?  (bf16x3 kernels, channel groups of 8)"""
        # (not the 14-pixel level, C1 = 256: the gather is repeated in each of its four output-channel slices, in a launch of few workgroups --
        # up1 12.0 -> 23.3 us at 8 images; up4 31.7 -> 27.0, up3 19.9 -> 19.3 us; up2, two slices: +4.8 us at 8 images, -3.5 at 16.
        # Same-box A/B of the threshold: profiles/r05_upb_fuse.txt)
        return bool(self.upb_fuse and self._b16 and su.taps == 1 and su.cout % 8 == 0 and su.cin <= self.upb_max_c1)

    def _upb_rows(self, su: ConvSpec) -> int:
        """Workgroups of that dgrad launch = rows of the bias-gradient sums it leaves (16 x 16-pixel tiles at the aligned sizes, 8 x 8 otherwise)."""
        t = 16 if (su.h % 16 == 0 and su.w % 16 == 0) else 8
        return self.N * ((su.h + t - 1) // t) * ((su.w + t - 1) // t)

    def _side_buf(self, pool: Dict[str, torch.Tensor], s: ConvSpec, c: int) -> torch.Tensor:
        """dzbuf / actbuf entry of layer s ([N,h,w,c] fp32 words), created on first use."""
        if s.name not in pool:
            pool[s.name] = torch.empty(self.N, s.h, s.w, c, dtype=torch.float32, device=self.dev)
        return pool[s.name]

    @staticmethod
    def _side_layer(s: ConvSpec) -> bool:
        """3x3 layers below the 16-pixel-aligned resolutions: separate dgrad + wgrad on the persistent conv kernel (the aligned ones run the
        fused / thin kernels, which stage input and dZ once for both gradients already)."""
        return s.taps == 9 and bool(s.h % 16 or s.w % 16)

    def _sums_from_epilogue(self, ca: L.ConvArgs, s: ConvSpec, kind: int, layer: str, dA: torch.Tensor, dA_ps: int, rows: Optional[int] = None):
        """The BatchNorm-backward sums of `layer` come out of the epilogue of the launch `ca` (of layer s), into the pass's sink -- rows of
        self.partials or the layer's accumulator -- and the following _bn_backward(layer) skips its own streaming pass over (dA, z).  kind 1: the
        launch's output is the complete dA; 2: it is dP, scattered into dA (max-pool backward) first.  rows: workgroups, if the caller fixed them."""
        ca.bwd_stats, ca.bwd_of, ca.stat_partials = kind, self._act_dz(layer, dA, dA_ps), L.ptr(self.partials)
        if rows is None:
            rows = self.lib.hpfg_conv_stat_rows(C.byref(ca))
        if rows <= 0 or rows * 2 * s.cin > self.partials.numel():
            raise RuntimeError(f"backward of {s.name}: {rows} rows of backward sums of {layer} do not fit the partials workspace")
        if self.bwd_route == ACC:
            ca.stat_partials, ca.stat_acc, ca.stat_shards = None, L.ptr(self.accb_of[layer]), self.acc_shards[layer]
        self._fused_rows[layer] = rows
        if kind == 2:
            self._pool_done.add(layer)

    def _dx_args(self, ca: L.ConvArgs, s: ConvSpec, g: L.Act, out: Optional[torch.Tensor], out2: Optional[torch.Tensor]) -> L.ConvArgs:
        """The input-gradient side of a launch: dX of layer s = conv-transpose of the dZ source g, into `out` (None: no dX, the first layer)."""
        ca.a0, ca.math, ca.out = g, self.math, L.ptr(out)
        if out is not None:
            ca.wpk = L.ptr(self.wpk16_d[s.name]) if self._b16 else L.ptr(self.wpk_d[s.name])
        ca.out_pstride, ca.Cout, ca.CoutPad = s.cin, s.cin, s.cin_pad
        if out2 is not None:          # [d(skip) | d(upsampled)] into two buffers
            ca.out2, ca.out_split, ca.out_pstride, ca.out2_pstride = L.ptr(out2), s.cin // 2, s.cin // 2, s.cin // 2
        ca.N, ca.H, ca.W, ca.taps = self.N, s.h, s.w, s.taps
        return ca

    def _fused_bwd(self, s: ConvSpec, g: L.Act, out: torch.Tensor, stats_for: Optional[str], out2: Optional[torch.Tensor]):
        """hpfg_fused_bwd: dX into `out` (/ `out2`), the weight-gradient slabs of layer s and -- with stats_for -- the BatchNorm-backward
        sums of the layer below, from one read of (dA, z) and one read of the layer input."""
        fa = L.FusedBwdArgs()
        fa.xa0, fa.xa1 = self.input_acts(s.name)
        fa.slab = L.ptr(self.slab_of[s.name])
        fa.Cin, fa.CinPad, fa.Cout, fa.CoutPad = s.cin, s.cin_pad, s.cout, s.cout_pad
        ca = self._dx_args(fa.d, s, g, out, out2)
        # _alloc_bwd sized the slab region and the reduction for `rows` workgroups: a kernel-form option (hpfg_set_option) switched since changes that
        rows, grid = self.fused_grid[s.name], self.lib.hpfg_fused_bwd_grid(C.byref(fa))
        if grid != rows:
            raise RuntimeError(f"fused_bwd[{s.name}]: {grid} workgroups, {rows} weight-gradient slabs allocated")
        if stats_for is not None and self.fuse_bwd_stats and s.cin == s.cin_pad and out2 is None:
            self._sums_from_epilogue(ca, s, 1, stats_for, out, s.cin, rows)
        self._call(self.lib.hpfg_fused_bwd, C.byref(fa), tag="fused_bwd:" + s.name)

    def _wgrad(self, s: ConvSpec, g: L.Act, stream: Optional[int] = None):
        """Weight gradient of layer s.  It is off the critical chain of backward (nothing downstream consumes it before the final
        slab reduction), so it is issued on a second HIP stream forked behind the kernels recorded so far and joined at the end."""
        # stream: the side stream _flush_deferred forked, for one of the deferred batches
        wa = L.WgradArgs()
        if s.name in self._act_live:      # the forward conv stored the input it staged
            wa.a0, wa.a1 = self._act_split(self.actbuf[s.name], s.cin, s.h, s.w), L.Act()
        else:
            wa.a0, wa.a1 = self.input_acts(s.name)
        wa.g = g
        wa.slab, wa.dw_oihw, wa.defer_reduce = L.ptr(self.slab_of[s.name]), L.ptr(self.grads[f"{s.name}.weight"]), 1
        wa.Cin, wa.CinPad, wa.Cout, wa.CoutPad = s.cin, s.cin_pad, s.cout, s.cout_pad
        wa.N, wa.H, wa.W, wa.taps = self.N, s.h, s.w, s.taps
        wa.S = self.lib.hpfg_wgrad_splits(self.N, s.h, s.w, s.cin_pad, s.cout_pad, s.taps)
        wa.math = self.math
        self._call(self.lib.hpfg_wgrad, C.byref(wa), tag="wgrad:" + s.name, stream=stream)

    def _dgrad(self, s: ConvSpec, g: L.Act, out: torch.Tensor, stats_for: Optional[str] = None, out2: Optional[torch.Tensor] = None,
               stage_out: Optional[torch.Tensor] = None, pool_of: Optional[str] = None, side_sums: Optional[torch.Tensor] = None):
        """out [N,h,w,cin] = conv-transpose of dZ with this layer's weights.
        stats_for: name of the BatchNorm layer whose activated output `out` is the COMPLETE gradient of (this conv is its only
        consumer): the bf16x3 kernel's epilogue then also leaves that layer's backward sums (_sums_from_epilogue)."""
        ca = self._dx_args(L.ConvArgs(), s, g, out, out2)
        if stage_out is not None:
            ca.stage_out = L.ptr(stage_out)
        if side_sums is not None:
            ca.side_sums = L.ptr(side_sums)
            rows = self.lib.hpfg_conv_stat_rows(C.byref(ca))
            if rows != self.csum_rows[s.name]:
                raise RuntimeError(f"dgrad[{s.name}]: {rows} workgroups, {self.csum_rows[s.name]} rows of bias-gradient sums allocated")
        # (not for the 32-channel slices of 16x16-pixel tiles: that instantiation is out of registers and the extra epilogue spills)
        spills = s.taps == 9 and s.cin_pad % 32 == 0 and s.h % 16 == 0 and s.w % 16 == 0
        fusable = self._b16 and self.fuse_bwd_stats and s.cin == s.cin_pad
        if stats_for is not None and fusable and (not spills or self.fuse_bwd_stats == 2):
            self._sums_from_epilogue(ca, s, 1, stats_for, out, s.cin)
        elif pool_of is not None and fusable and self._side_layer(s) and out2 is None:
            # `out` would be dP, the gradient w.r.t. MaxPool2d(2) of layer pool_of's activation: the epilogue scatters it into that layer's
            # gradient (arg-max of the 2 x 2 window) and takes the BatchNorm-backward sums of the completed gradient -- hpfg_bn_bwd_reduce_pool's
            # pass, without its launch on the chain
            self._sums_from_epilogue(ca, s, 2, pool_of, self.dA[pool_of], self.dA_ps[pool_of])
        self._call(self.lib.hpfg_conv_fwd, C.byref(ca), tag="dgrad:" + s.name)

    def _slab_reduce(self, lo: int, hi: int, stream=None):
        """Sum the weight-gradient slabs of descriptors [lo, hi) into the gradient buffer (one launch)."""
        if hi <= lo:
            return
        self._call(self.lib.hpfg_slab_reduce_multi, *self.slabs.sub(lo, hi), tag="slab_reduce", stream=stream)

    def _csum(self, dlogits: torch.Tensor, stream: Optional[int] = None):
        """out_conv's bias gradient: per-block channel sums of dlogits (rows of the final slab reduction)."""
        s = self.specs["decoder.out_conv"]
        self._call(self.lib.hpfg_channel_sum_partials, L.ptr(dlogits), self.ncls, self.N * s.h * s.w, self.ncls, L.ptr(self.csum_part[s.name]), tag="csum:" + s.name, stream=stream)

    def _flush_deferred(self, lo: int, hi: int):
        """queued weight gradients -> side stream, followed there by the slab reduction of descriptors [lo, hi) (all their producers -- these
        launches and fused kernels already queued on the main stream -- are ordered before it by the fork)"""
        if self._deferred is None:
            return
        side = self._fork_side().cuda_stream
        if self._csum_pending is not None:          # out_conv's bias sums ride along with the first batch
            self._csum(self._csum_pending, side)
            self._csum_pending = None
        batches = [(self._deferred, lo, hi)]
        if hi == self._n_enc_desc and lo + 2 < hi and len(self._deferred) == hi - lo:
            # the deeper levels first, their slabs reduced beside the last level's weight gradients: the serial piece at the stream's
            # end -- it finished AFTER the main chain -- shrinks from 58 to ~20 us (with the reduction below: mt -0.8 %)
            batches = [(self._deferred[:-2], lo + 2, hi), (self._deferred[-2:], lo, lo + 2)]
        for layers, a, b in batches:
            for s_, g_ in layers:
                self._wgrad(s_, g_, side)
            self._slab_reduce(a, b, side)
        self._side_used = True

    def _bwd_head(self, dlogits: torch.Tensor):
        """out_conv: both gradients + the backward sums of the last decoder block, and the bias sums."""
        s = self.specs["decoder.out_conv"]
        g = self._act_plain(dlogits, self.ncls, s.h, s.w)
        if self.marks is not None:
            self.marks.calib(self._stream())          # (what a bracket costs by itself, measured where backward starts)
        if self._deferred is None:
            self._csum(dlogits)
        else:      # nothing on the chain of backward reads those rows -- they go out with the decoder's queued weight gradients on the side stream,
            self._csum_pending = dlogits      # instead of 11 us at the head of the critical chain
        self._wgrad_dgrad(s, g, self.dA["decoder.up4.conv.conv_conv.4"], "decoder.up4.conv.conv_conv.4")

    def _bwd_decoder_block(self, k: int, sole_consumer: bool):
        """Decoder block k: conv 4, conv 0 (-> dSkip | dUp), upsample backward + 1x1 conv, down to dA of the block output below.
        sole_consumer: the 1x1 conv is the only consumer of that output (the bottleneck also feeds the dense head of UNet_Plus)."""
        sp = self.specs
        p = f"decoder.up{k}.conv.conv_conv"
        s2, s1, su = sp[f"{p}.4"], sp[f"{p}.0"], sp[f"decoder.up{k}.conv1x1"]
        g2 = self._bn_backward(s2)
        self._wgrad_dgrad(s2, g2, self.dA[s1.name], s1.name)
        g1 = self._bn_backward(s1)
        c2 = su.cout
        self._wgrad_dgrad(s1, g1, self.dcat[k], out2=self.dup.get(k))      # [dSkip | dUp], or dSkip and dUp in buffers of their own
        if k in self.dup:
            dup, dup_ps = self.dup[k], c2
        else:
            dup, dup_ps = self.dcat[k].view(-1)[c2:], 2 * c2   # channel offset c2, pixel stride 2*c2
        prev = enc_prefix(4) + ".4" if k == 1 else f"decoder.up{k - 1}.conv.conv_conv.4"
        stats_prev = prev if sole_consumer else None
        gu = self._act_plain(self.dU[k], c2, su.h, su.w)
        if self._upb_on(su):
            # the dgrad gathers the upsample backward while it stages (and leaves dU + the bias-gradient rows for the weight gradient / the
            # slab reduction): one launch of the chain instead of two, dU written once and read once less
            gsrc = L.Act()
            gsrc.z, gsrc.mode, gsrc.C, gsrc.Hs, gsrc.Ws, gsrc.pstride = L.ptr(dup), L.ACT_UPBWD, c2, su.h, su.w, dup_ps
            self._dgrad(su, gsrc, self.dA[prev], stats_prev, stage_out=self.dU[k], side_sums=self.csum_part[su.name])
            if self._deferred is not None:
                self._deferred.append((su, gu))
            else:
                self._wgrad(su, gu)
        else:
            # (+ per-workgroup channel sums of dU: the 1x1 conv's bias gradient)
            self._call(self.lib.hpfg_upsample2x_bwd_sums, L.ptr(dup), dup_ps, L.ptr(self.dU[k]), self.N, su.h, su.w, c2, L.ptr(self.csum_part[su.name]), tag="upbwd:" + su.name)
            self._wgrad_dgrad(su, gu, self.dA[prev], stats_prev)

    def _bwd_encoder_level(self, lvl: int):
        """Encoder level lvl: conv 4, conv 0, down to dP (the gradient w.r.t. the max-pooled block output below)."""
        p = enc_prefix(lvl)
        s2, s1 = self.specs[f"{p}.4"], self.specs[f"{p}.0"]
        # a block output below the bottleneck also fed the max-pool of the next level: its dP is folded in by the reduction pass
        g2 = self._bn_backward(s2, self.dP[lvl + 1] if (lvl < 4 and s2.name not in self._pool_done) else None)
        self._wgrad_dgrad(s2, g2, self.dA[s1.name], s1.name)
        g1 = self._bn_backward(s1)
        if lvl > 0:      # (pool_fuse: the max-pool backward into the block output below rides in this dgrad's epilogue)
            self._wgrad_dgrad(s1, g1, self.dP[lvl], pool_of=(enc_prefix(lvl - 1) + ".4") if self.pool_fuse else None)
        elif s1.name in self.fused_grid:
            self._fused_bwd(s1, g1, None, None, None)
        else:
            self._wgrad(s1, g1)

    def backward(self, dlogits: torch.Tensor, dfeat4: Optional[torch.Tensor] = None, bucket_cb=None):
        """dlogits: [N,H,W,ncls] contiguous.  dfeat4: optional gradient w.r.t. the activated bottleneck [N,h,w,256].
        bucket_cb: optional callable(i); called with 0 once every DECODER parameter gradient is final (queued on the current stream:
        decoder slabs reduced by a launch of their own) and with 1 after the encoder's -- data parallel: the decoder bucket is
        all-reduced on a side stream while the encoder half of backward still computes (hpfg_amd.parallel.GradBuckets).
        Writes every parameter gradient of encoder/decoder into self.grads (overwrite).  Biases of convs that feed a
        train-mode BatchNorm have an exactly zero gradient (the batch mean removes them); their slots are never written and
        rely on the zero-initialised gradient buffer."""
        assert self.bwd_ready, "backward() needs a preceding train-mode forward()"
        assert dlogits.is_contiguous() and tuple(dlogits.shape) == (self.N, self.H, self.W, self.ncls)
        self._alloc_bwd()
        self.bwd_route = bn_route(True, self.math, self.bn_acc_on, self.peer is not None, self.world, self.force_sync)
        if self.bwd_route == ACC:
            if self._accb_dirty:          # a backward pass that did not reach its finalize launch (an exception): start from zero
                self.accb_all.zero_()
            self._accb_dirty = True
        # ONE fork for the decoder's separate weight gradients (the channel-rich layers and the 1x1 convs; the thin layers' are fused with their
        # dgrad): they are queued while the decoder half back-propagates and run on the side stream beside the encoder half -- everything they
        # read (dA, z, the BatchNorm tables of their layers) stays in place until the next forward.  A fork / join per layer cost more than it
        # returned (round 1; removed); this is one of each.  Not with the data-parallel buckets: the decoder's gradients must be final at the
        # bucket boundary.
        defer = bool(self.defer_wgrad and bucket_cb is None)
        self._deferred = [] if defer else None
        self._pool_done, self._csum_pending = set(), None      # (nothing a pass that raised left behind)
        self._bwd_head(dlogits)
        for k in range(4, 0, -1):      # decoder blocks, last to first
            self._bwd_decoder_block(k, sole_consumer=k > 1 or dfeat4 is None)
        if dfeat4 is not None:
            self.dA[enc_prefix(4) + ".4"].add_(dfeat4)
        self._flush_deferred(self._n_enc_desc, len(self.slabs.host))
        self._deferred = [] if defer else None      # second batch: the channel-rich encoder layers, beside the thin layers' fused kernels
        if bucket_cb is not None:
            self._join_side()
            self._slab_reduce(self._n_enc_desc, len(self.slabs.host))
            self._finalize_bwd_all(self._n_enc_bn, len(self.bn_layers))      # the decoder's dgamma / dbeta are part of bucket 0
            bucket_cb(0)
        for lvl in range(4, -1, -1):      # encoder levels, deepest first
            self._bwd_encoder_level(lvl)
            if lvl == 2:
                self._flush_deferred(self._n_thin_enc_desc, self._n_enc_desc)
                self._deferred = None
        if defer:
            # the thin encoder layers' slabs come from fused kernels on THIS stream: reduce them before the join, beside the side stream's last
            # launches, instead of behind the join and the finalize launch
            self._slab_reduce(0, self._n_thin_enc_desc)
        self._join_side()
        # every dZ consumer of the pass (the queued weight gradients on the side stream included) has been ordered before this point
        self._finalize_bwd_all(0, self._n_enc_bn if bucket_cb is not None else len(self.bn_layers))
        self._accb_dirty = False
        if bucket_cb is not None:
            self._slab_reduce(0, self._n_enc_desc)
            bucket_cb(1)
        elif not defer:
            self._slab_reduce(0, len(self.slabs.host))
        # (defer: the thin layers' slabs were reduced in front of the join above, everything else on the side stream)
        self.bwd_ready = False
