"""CPU: the two entry points of csrc/bn_stencil_fused.hip are declared and exported, and their host-side checks refuse bad arguments
before any launch (no GPU is touched: every call here fails a check).  Pointers are fake but 16-byte aligned; they are never
dereferenced on the host."""
import ctypes

import pytest

ERR_ARG = -1
P = ctypes.c_void_p(0x1000)            # aligned, non-null
ODD = ctypes.c_void_p(0x1008)          # not 16-byte aligned


@pytest.fixture(scope="module")
def L():
    from egm_unet_amd import build
    build.build(verbose=False)
    from egm_unet_amd._lib import lib
    return lib()


def test_entries_are_declared_and_exported(L):
    from egm_unet_amd._lib import parse_header
    protos = parse_header()
    for name, nargs in (("egm_bn_act_hp_fwd", 15), ("egm_bn_act_upcat_fwd", 18)):
        assert name in protos and len(protos[name][1]) == nargs, name
        assert protos[name][0] is ctypes.c_int
        assert hasattr(L.cdll, name)


def _hp(L, dtype=1, y=P, ldy=8, scale=P, shift=P, act=1, z=P, ldz=8, edge=P, lde=8, N=1, H=4, W=4, C=8):
    rc = L.cdll.egm_bn_act_hp_fwd(dtype, y, ldy, scale, shift, act, z, ldz, edge, lde, N, H, W, C, None)
    return rc, L.cdll.egm_last_error().decode()


def _up(L, dtype=1, skip=P, lds=8, low=P, ldl=8, scale=P, shift=P, act=1, out=P, ldo=16, N=1, Hs=4, Ws=4, Cs=8, Hl=2, Wl=2, Cl=8):
    rc = L.cdll.egm_bn_act_upcat_fwd(dtype, skip, lds, low, ldl, scale, shift, act, out, ldo, N, Hs, Ws, Cs, Hl, Wl, Cl, None)
    return rc, L.cdll.egm_last_error().decode()


@pytest.mark.parametrize("bad", [dict(y=None), dict(z=None), dict(edge=None), dict(scale=None), dict(shift=None), dict(y=ODD), dict(z=ODD),
                                 dict(edge=ODD), dict(C=12, ldy=16, ldz=16, lde=16), dict(C=0), dict(C=16), dict(ldy=4), dict(C=16, ldy=16, ldz=8, lde=16),
                                 dict(C=16, ldy=16, ldz=16, lde=8), dict(ldz=12), dict(N=0), dict(H=0), dict(W=0), dict(act=4), dict(act=-1),
                                 dict(dtype=0), dict(dtype=7)])
def test_bn_act_hp_fwd_refuses(L, bad):
    rc, msg = _hp(L, **bad)
    assert rc == ERR_ARG and msg.startswith("bn_act_hp_fwd"), (bad, rc, msg)


@pytest.mark.parametrize("bad", [dict(low=None), dict(out=None), dict(scale=None), dict(shift=None), dict(skip=ODD), dict(low=ODD), dict(out=ODD),
                                 dict(Cl=12, ldl=16, ldo=24), dict(Cs=12, lds=16, ldo=24), dict(Cs=0), dict(Cl=0), dict(ldl=4), dict(lds=4),
                                 dict(ldo=8), dict(ldo=20), dict(Hs=3), dict(Ws=3), dict(Hl=3), dict(Wl=3), dict(N=0), dict(Hl=0), dict(Wl=0),
                                 dict(act=4), dict(dtype=0), dict(skip=None, Cs=12)])
def test_bn_act_upcat_fwd_refuses(L, bad):
    rc, msg = _up(L, **bad)
    assert rc == ERR_ARG and msg.startswith("bn_act_upcat_fwd"), (bad, rc, msg)
