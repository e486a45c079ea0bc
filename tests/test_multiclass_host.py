"""CPU: the host side of the 5..16-class range -- the two Synapse-shaped configs build a model / optimizer / scheduler, hpfg_loss_nsum is
exported with its two values, and HpfgLossArgs kept its layout."""
import ctypes
import os
import re

import pytest

from hpfg_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["unet_30k_224x224_Synapse.yaml", "ict-medseg_unet_30k_224x224_Synapse.yaml"])
def test_synapse_configs_build(name):
    from hpfg_amd.model import build_model
    from hpfg_amd.utils import build_lr_scheduler, build_optimizer, loadyaml
    args = loadyaml(os.path.join(ROOT, "config", name))
    assert args.num_classes == 9 and args.model == "unet" and args.opt == "sgd" and args.in_channels == 1
    assert args.datasets in ("sup_synthetic", "synthetic")
    model = build_model(args=args)
    assert model.num_classes == 9 and model.in_channels == 1
    opt = build_optimizer(args=args, model=model)
    sched = build_lr_scheduler(args=args, optimizer=opt)
    # (the schedulers step once at construction, as the reference's do: cosine starts at its table's last entry, medical just above lr)
    assert sched is not None and 0.0 < opt.param_groups[0]["lr"] <= args.lr * 1.001
    opt.step()
    sched.step()
    assert abs(opt.param_groups[0]["lr"] - args.lr) < 1e-9          # the first scheduled value of either law is the base rate


def test_loss_nsum_is_exported_with_two_values():
    lib = L.load()
    assert [lib.hpfg_loss_nsum(c) for c in (2, 3, 4)] == [32, 32, 32] and L.LOSS_NSUM == 32
    wide = {lib.hpfg_loss_nsum(c) for c in range(5, 17)}
    assert len(wide) == 1
    (w,) = wide
    assert w >= 8 + 6 * 16 and w <= 512          # six scalars, six blocks of 16; within a peer mailbox slot (512 values per rank)
    src = open(os.path.join(ROOT, "include", "hpfg_hip.h")).read()
    assert int(re.search(r"#define HPFG_LOSS_NSUM_WIDE (\d+)", src).group(1)) == w
    assert int(re.search(r"#define HPFG_LOSS_NSUM (\d+)", src).group(1)) == 32


_CTYPES = {"const float*": ctypes.c_void_p, "float*": ctypes.c_void_p, "const uint8_t*": ctypes.c_void_p, "int32_t": ctypes.c_int32}


def test_loss_args_struct_size_unchanged():
    """sizeof(LossArgs) computed from the header's own field list (as tests/test_abi.py reads it) and against the layout the C <= 4 kernels
    have always been launched with: 9 pointers, 10 int32, 1 pointer."""
    src = open(os.path.join(ROOT, "include", "hpfg_hip.h")).read()
    body = re.search(r"typedef struct HpfgLossArgs \{(.*?)\} HpfgLossArgs;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = [n.strip() for n in decl.split(",")]
        typ, first = names[0].rsplit(None, 1)
        if first.startswith("*"):
            typ, first = typ + "*", first[1:]
        for n in [first] + names[1:]:
            fields.append((n.lstrip("*"), _CTYPES[typ]))

    class FromHeader(ctypes.Structure):
        _fields_ = fields

    assert [f[0] for f in fields] == [f[0] for f in L.LossArgs._fields_]
    assert ctypes.sizeof(FromHeader) == ctypes.sizeof(L.LossArgs) == 9 * 8 + 10 * 4 + 8
