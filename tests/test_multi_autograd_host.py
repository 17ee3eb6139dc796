"""CPU: the split ragged multi-slide entry points (toad_mil_multi_fwd_f32 / toad_mil_multi_bwd_f32, ABI 14) validate their arguments
before touching the device, and TOAD_fc_mtl_concat.forward_batch refuses what the batched route cannot run before any device call."""
import ctypes
import inspect

import pytest
import torch


def _lib():
    from toad_amd import _lib as L
    return L.load()


def test_multi_fwd_bwd_report_argument_errors_without_a_gpu():
    lib = _lib()
    assert lib.toad_abi_version() == 15
    err = lambda: lib.toad_last_error().decode()              # noqa: E731
    one = ctypes.c_void_p(1 << 21)                            # non-null, aligned fake pointers: every check below comes before a device access
    big = 1 << 40
    p12 = (ctypes.c_void_p * 12)(*([1 << 21] * 12))
    offs = (ctypes.c_int64 * 4)(0, 100, 300, 301)
    fwd = lambda pr, o, b, ab=big, sb=big, drop=0.0: lib.toad_mil_multi_fwd_f32(pr, one, o, b, one, 18, 384, drop, 0, one, ab, one, sb, None)  # noqa: E731
    assert fwd(None, offs, 3) == -1 and "null pointer" in err()
    assert fwd(p12, None, 3) == -1 and "null pointer" in err()
    assert fwd(p12, offs, 0) == -1 and "B must be in [1, 4096]" in err()
    assert fwd(p12, offs, 4097) == -1 and "B must be in [1, 4096]" in err()
    assert fwd(p12, (ctypes.c_int64 * 4)(1, 100, 300, 301), 3) == -1 and "offsets[0] must be 0" in err()
    assert fwd(p12, (ctypes.c_int64 * 4)(0, 100, 100, 301), 3) == -1 and "slide 1 is empty" in err()
    assert fwd(p12, (ctypes.c_int64 * 2)(0, 1 << 20), 1) == -2 and "unsupported shape" in err()      # 2^20 rows: beyond one NT launch
    assert fwd(p12, offs, 3, drop=1.0) == -1 and "drop_p" in err()
    assert fwd(p12, offs, 3, ab=16) == -3 and "arena too small" in err()
    assert fwd(p12, offs, 3, sb=16) == -3 and "scratch too small" in err()
    assert lib.toad_mil_multi_fwd_f32(p12, ctypes.c_void_p((1 << 21) + 4), offs, 3, one, 18, 384, 0.0, 0, one, big, one, big, None) == -4 \
        and "aligned" in err()
    p12[5] = None
    assert fwd(p12, offs, 3) == -1 and "slot 5" in err()
    p12[5] = 1 << 21
    g12 = (ctypes.c_void_p * 12)(*([1 << 21] * 12))
    bwd = lambda gr, dl, b=3, ab=big, sb=big: lib.toad_mil_multi_bwd_f32(p12, gr, 0.0, one, offs, b, 18, 384, 0.0, 0, one, ab, dl, one, None,  # noqa: E731
                                                                           None, one, sb, None)
    assert bwd(g12, None) == -1 and "null pointer" in err()                 # dlogits is required (dA / dMcat are optional)
    assert bwd(g12, one, b=0) == -1 and "B must be in [1, 4096]" in err()
    assert bwd(g12, one, ab=16) == -3 and "arena too small" in err()
    assert bwd(g12, one, sb=16) == -3 and "scratch too small" in err()
    g12[11] = None
    assert bwd(g12, one) == -1 and "gradient slot 11" in err()


def test_multi_arena_layout_and_sizes():
    lib = _lib()
    n, nb, c, d = 100000, 52, 18, 384
    assert lib.toad_mil_multi_arena_bytes(n, 0, c, d) == 0 and lib.toad_mil_multi_arena_bytes(n, 4097, c, d) == 0
    assert lib.toad_mil_multi_arena_bytes(n, nb, c, 100) == 0 and lib.toad_mil_multi_scratch_bytes(0, nb, c, d) == 0
    offs = (ctypes.c_int64 * 11)()
    assert lib.toad_mil_multi_arena_layout(n, nb, c, d, offs) == 0
    o = list(offs)
    one = (ctypes.c_int64 * 18)()
    assert lib.toad_mil_arena_layout(n, c, d, one) == 0
    assert o[:4] == list(one)[:4]                                            # H1, H, P, A_raw where the one-slide arena keeps them
    assert all(b > a for a, b in zip(o, o[1:])) and all(x % 256 == 0 for x in o)
    assert o[5] - o[4] >= nb * 2 * 513 * 4 and o[6] - o[5] >= nb * c * 4    # dense [B, 2, 513] features, [B, C] logits
    assert lib.toad_mil_multi_arena_bytes(n, nb, c, d) >= o[10] + nb * 8
    assert lib.toad_mil_multi_arena_bytes(n, nb, c, d) > lib.toad_mil_arena_bytes(n, c, d)
    assert lib.toad_mil_multi_scratch_bytes(n, nb, c, d) > lib.toad_mil_scratch_bytes(n, c, d)
    assert lib.toad_mil_multi_arena_layout(n, 0, c, d, offs) == -2


def test_forward_batch_exists_with_the_documented_signature():
    from toad_amd import TOAD_fc_mtl_concat, functional
    sig = inspect.signature(TOAD_fc_mtl_concat.forward_batch)
    assert list(sig.parameters) == ["self", "bags", "sexes", "return_features"]
    assert sig.parameters["return_features"].default is False
    assert issubclass(functional.ToadMILBatch, torch.autograd.Function)
    from toad_amd import ops
    assert list(inspect.signature(ops.mil_multi_fwd).parameters)[:6] == ["w", "bags_or_xcat", "sex", "drop_p", "seed", "offsets"]
    assert list(inspect.signature(ops.mil_multi_bwd).parameters)[:8] == ["w", "grads", "beta", "xcat", "offsets", "arena", "dlogits", "dsite"]


def test_forward_batch_refuses_before_any_device_call():
    """CPU tensors throughout: a device call would raise RuntimeError ("no CPU fallback"), so each ValueError / TypeError below was raised first."""
    from toad_amd import TOAD_fc_mtl_concat, ops
    m = TOAD_fc_mtl_concat(n_classes=4)
    x = torch.randn(5, 1024)
    s = torch.tensor([1.0])
    with pytest.raises(ValueError, match="one sex entry per bag"):
        m.forward_batch([x, x], [s])
    with pytest.raises(ValueError, match="empty bag"):
        m.forward_batch([x, torch.empty(0, 1024)], [s, s])
    with pytest.raises(ValueError, match=r"\[N, 1024\]"):
        m.forward_batch([torch.randn(5, 512)], [s])
    with pytest.raises(TypeError, match="PreparedBag"):
        m.forward_batch([ops.PreparedBag(torch.empty(16, dtype=torch.uint8), torch.empty(1), 64, 1024)], [s])
    with pytest.raises(ValueError, match="1048575 rows per call"):
        m.forward_batch([torch.empty(1, 1024).expand(1 << 20, 1024)], [s])          # (a stride-0 view: no memory behind the 2^20 rows)
    with pytest.raises(ValueError, match="4096 slides per call"):
        m.forward_batch([x] * 4097, [s] * 4097)
    with pytest.raises(ValueError, match="no gradient with respect to the bags or the sexes"):
        m.forward_batch([torch.randn(5, 1024, requires_grad=True)], [s])
    with pytest.raises(ValueError, match="no gradient with respect to the bags or the sexes"):
        m.forward_batch([x], [torch.tensor([1.0], requires_grad=True)])
    with pytest.raises(ValueError, match="no gradient with respect to the bags or the sexes"):
        m.forward_batch([x], torch.tensor([1.0], requires_grad=True))
    assert m.forward_batch([], []) == []
    with pytest.raises(RuntimeError, match="no CPU fallback"):                      # a valid batch gets as far as the device check
        m.forward_batch([x], [s])
