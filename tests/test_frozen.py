"""Frozen-weight inference, host side (no device): the frozen arena's size and composition, uwm_freeze's argument checks and the
Python freeze() precondition.  The GPU behaviour is in tests/test_frozen_gpu.py."""
import ctypes as C

import pytest
import torch


@pytest.fixture(scope="module")
def U():
    import __graft_entry__ as g
    g.build()
    import unet_watermark_amd as U
    return U


def _lookup(L, m, key):
    off, cnt = C.c_longlong(), C.c_longlong()
    L.check(L.lib().uwm_debug_lookup(m._h, key.encode(), C.byref(off), C.byref(cnt)))
    return off.value, cnt.value


def _names(L, m):
    """state_dict prefixes of the model's BatchNorms and convolutions"""
    bns = [n[:-len(".running_mean")] for n, kind, *_ in m._infos if kind == L.KIND_BN_MEAN]
    convs = [n[:-len(".weight")] for n, kind, *_ in m._infos if kind == L.KIND_CONV_W]
    return bns, convs


def test_frozen_bytes_follow_from_the_model_alone(U):
    """Expected composition of the arena: 2 floats (scale, shift) per BatchNorm channel + one forward bank slot per layer that has
    one (stem included), each part rounded up to whole 64-float lines; nothing of the backward (dgrad banks, dgrad repacks) and
    none of the statistics scratch.  So for Unet-resnet34 it is no larger than the workspace's fixed region minus the dgrad items."""
    L = U._lib
    lib = L.lib()
    for arch, enc in (("Unet", "resnet34"), ("UnetPlusPlus", "resnet18"), ("Unet", "efficientnet-b0")):
        m = getattr(U, arch)(enc)
        b0 = lib.uwm_frozen_bytes(m._h)
        assert b0 > 0 and b0 % 4 == 0
        assert lib.uwm_workspace_bytes(m._h, 2, 128, 128, 0) > 0
        assert lib.uwm_frozen_bytes(m._h) == b0
        assert lib.uwm_workspace_bytes(m._h, 8, 512, 512, 0) > 0
        assert lib.uwm_frozen_bytes(m._h) == b0
        bns, convs = _names(L, m)
        bn_floats = sum(_lookup(L, m, "bnf:" + b)[1] for b in bns)
        assert bn_floats == 2 * sum(s[0] for n, kind, a, o, s, st in m._infos if kind == L.KIND_BN_MEAN)
        slots = [_lookup(L, m, "wu:" + c)[1] for c in convs]
        nslots = sum(1 for s in slots if s > 0)
        if enc.startswith("resnet"):
            assert nslots > 0 and _lookup(L, m, "wu:encoder.conv1")[1] > 0            # the stem's fp16x3 bank has a slot
        lo = bn_floats + sum(slots)
        assert lo <= b0 // 4 <= lo + 64 * (nslots + 1), (lo, b0 // 4, nslots)
        fixed = _lookup(L, m, "fixed")[1]
        dgrad = sum(_lookup(L, m, "wd:" + c)[1] + _lookup(L, m, "wud:" + c)[1] for c in convs)
        assert dgrad > 0
        assert b0 // 4 <= fixed - dgrad, (b0 // 4, fixed, dgrad)


def test_uwm_freeze_rejects_bad_calls(U):
    L = U._lib
    lib = L.lib()
    m = U.Unet("resnet18")
    need = lib.uwm_frozen_bytes(m._h)
    buf = (C.c_char * 64)()                                      # never written: every call below fails before any launch
    ptr = C.c_void_p((C.addressof(buf) + 15) & ~15)

    def err():
        return lib.uwm_last_error().decode()

    assert lib.uwm_is_frozen(m._h) == 0
    assert lib.uwm_freeze(m._h, ptr, need, 2, 128, 128, None) != 0                 # no arenas bound
    assert "uwm_bind" in err()
    assert lib.uwm_is_frozen(m._h) == 0
    assert lib.uwm_freeze(m._h, ptr, need - 4, 2, 128, 128, None) != 0             # short arena
    assert "too small" in err()
    assert lib.uwm_is_frozen(m._h) == 0
    assert lib.uwm_freeze(m._h, ptr, need, 2, 100, 128, None) != 0                 # H % 32 != 0
    assert "divisible by 32" in err()
    assert lib.uwm_is_frozen(m._h) == 0
    assert lib.uwm_freeze(m._h, None, need, 2, 128, 128, None) != 0
    assert err()
    assert lib.uwm_frozen_serves(m._h, 2, 128, 128) == 0
    assert lib.uwm_prep_launches(m._h) == 0
    assert lib.uwm_unfreeze(m._h) == 0


def test_freeze_needs_eval_mode_and_a_device(U):
    m = U.Unet("resnet18")
    assert m.training and not m.frozen
    with pytest.raises(RuntimeError, match="eval mode"):
        m.freeze()
    assert not m.frozen
    m.eval()
    with pytest.raises(RuntimeError, match="HIP device"):
        m.freeze()
    assert not m.frozen
    with pytest.raises(RuntimeError):
        m.predict_u8(torch.zeros(1, 32, 32, 3, dtype=torch.uint8), (0.5,) * 3, (0.25,) * 3)
