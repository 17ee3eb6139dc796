"""CPU: the one argument builder behind the whole-slide wrappers (ops._mil_args). For each of the 15 entries - step / fwd / bwd for an fp32,
an fp16 and a prepared bag, multi_step / multi_fwd / multi_bwd for fp32 and fp16 - the name it resolves is in the ctypes table and the tuple
it builds has that entry's arity, with a value ctypes takes in every position. No tensor, no library, no GPU."""
import ctypes

import pytest

from toad_amd import _lib as L
from toad_amd import ops

ONE_SLIDE, MULTI = ("step", "fwd", "bwd"), ("multi_step", "multi_fwd", "multi_bwd")
ENTRIES = [(f, k) for f in ONE_SLIDE for k in (ops.KIND_F32, ops.KIND_F16, ops.KIND_PREPARED)] + \
          [(f, k) for f in MULTI for k in (ops.KIND_F32, ops.KIND_F16)]
ARRAYS = {"w": (ctypes.c_void_p * 12)(), "g": (ctypes.c_void_p * 12)(), "offsets": (ctypes.c_int64 * 4)(0, 64, 65, 320),
          "events": (ctypes.c_void_p * 18)()}
FLOATS = ("beta", "w_cls", "w_site", "drop_p")
NONE = ("logits", "slog", "da_ext", "dmcat_ext", "dsex")        # optional pointers, absent


def _values(family, kind, dx=None):
    """One placeholder per field of the family: what the wrappers pass, with made-up addresses and sizes."""
    vals = []
    for i, field in enumerate(ops._MIL_FIELDS[family]):
        name = field.lstrip("*")
        if name == "bag":
            vals.append((0x1000, 0x2000) if kind == ops.KIND_PREPARED else (0x1000,))
        elif name == "dx":
            vals.append(dx)
        elif name in ARRAYS:
            vals.append(ARRAYS[name])
        elif name in FLOATS:
            vals.append(0.25)
        else:
            vals.append(None if name in NONE else 0x100 * (i + 1))
    return tuple(vals)


def test_the_fifteen_entries():
    assert len(ENTRIES) == 15 and len(set(ENTRIES)) == 15
    names = {ops._mil_args(f, k, _values(f, k))[0] for f, k in ENTRIES}
    assert names == {n for n in L.SIGNATURES if n.startswith("toad_mil_") and n.endswith("_f32")}, "every whole-slide entry of the table, no other"


@pytest.mark.parametrize("family,kind", ENTRIES)
def test_argument_list_matches_the_signature(family, kind):
    name, args = ops._mil_args(family, kind, _values(family, kind))
    assert name in L.SIGNATURES, name
    types = L.SIGNATURES[name][1]
    assert len(args) == len(types), (name, len(args), len(types))
    for pos, (a, t) in enumerate(zip(args, types)):
        if t is L.P:
            assert a is None or isinstance(a, (int, ctypes.Array)), (name, pos, a)
        elif t is L.F:
            assert isinstance(a, float), (name, pos, a)
        else:
            assert t in (L.I, L.I64, L.SZ, L.U64) and isinstance(a, int) and not isinstance(a, bool), (name, pos, a)
    # the kinds differ in the bag position and the fp32-only argument, nowhere else
    ref = ops._mil_args(family, ops.KIND_F32, _values(family, ops.KIND_F32))[1]
    extra = [f for f in ops._MIL_FIELDS[family] if f[0] == "*"]
    assert len(ref) - len(args) == (len(extra) if kind != ops.KIND_F32 else 0) - (kind == ops.KIND_PREPARED)
    assert len(extra) == (1 if family in ONE_SLIDE else 0)
    if family in MULTI:
        assert args == ref


def test_arguments_keep_their_places():
    """Distinct placeholders: each value lands where the header puts its field (include/toad_hip.h), for the three step lists."""
    f = ops._MIL_FIELDS["step"]
    for kind, bag in ((ops.KIND_F32, ("X",)), (ops.KIND_F16, ("X",)), (ops.KIND_PREPARED, ("PLANES", "AMAX"))):
        vals = tuple(bag if n == "bag" else n.lstrip("*") for n in f)
        _, args = ops._mil_args("step", kind, vals)
        want = list(f[:3]) + list(bag) + list(f[4:14]) + (["x_amax"] if kind == ops.KIND_F32 else []) + list(f[15:])
        assert list(args) == want, (kind, args)


@pytest.mark.parametrize("kind", [ops.KIND_F16, ops.KIND_PREPARED])
def test_no_gradient_for_a_bag_that_is_not_fp32(kind):
    with pytest.raises(ValueError, match="no gradient with respect to an fp16 / prepared bag"):
        ops._mil_args("bwd", kind, _values("bwd", kind, dx=0x5000))
    name, args = ops._mil_args("bwd", ops.KIND_F32, _values("bwd", ops.KIND_F32, dx=0x5000))
    assert name == "toad_mil_bwd_f32" and 0x5000 in args
    ops._mil_args("bwd", kind, _values("bwd", kind))           # without dx the other kinds are fine
