"""CPU: the mask clean-up's host side -- the MaskCleanup value object, the numpy oracle of tests/cleanup_oracle.py against scipy (where
scipy is installed), the argument checks of the C entry points that need no device, and the stand-alone host program that runs the
kernels' union-find core (csrc/ccl_core.h) on the CPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cleanup_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- MaskCleanup
def test_mask_cleanup_validation_and_resolve():
    from egm_unet_amd.postprocess import MaskCleanup
    from egm_unet_amd import ensemble
    assert ensemble.MaskCleanup is MaskCleanup                              # re-exported
    d = MaskCleanup()
    assert (d.min_area, d.keep_largest, d.max_hole, d.connectivity) == (0, False, 0, 8)
    assert d.neutral and MaskCleanup(min_area=1).neutral and MaskCleanup(connectivity=4).neutral
    assert not MaskCleanup(min_area=2).neutral and not MaskCleanup(keep_largest=True).neutral and not MaskCleanup(max_hole=1).neutral
    assert not MaskCleanup(min_area=0.001).neutral
    assert d.resolve(565, 753) == (0, 0, 0)
    r = MaskCleanup(min_area=0.002, keep_largest=True, max_hole=200)
    assert r.resolve(565, 753) == (int(np.ceil(0.002 * 565 * 753)), 1, 200) == (851, 1, 200)
    assert MaskCleanup(min_area=7, max_hole=0.5).resolve(3, 3) == (7, 0, 5)        # ceil(4.5)
    assert MaskCleanup(min_area=0.25).resolve(4, 4) == (4, 0, 0)                  # an exact product is not rounded up
    assert all(isinstance(v, int) for v in r.resolve(10, 10))
    for bad in (dict(min_area=-1), dict(max_hole=-3), dict(min_area=1.0), dict(min_area=0.0), dict(max_hole=1.5), dict(max_hole=-0.1),
                dict(connectivity=5), dict(connectivity=6), dict(connectivity=0), dict(min_area="3")):
        with pytest.raises(ValueError):
            MaskCleanup(**bad)
    with pytest.raises(AttributeError):                                     # immutable
        r.min_area = 3
    assert r == MaskCleanup(min_area=0.002, keep_largest=True, max_hole=200) and hash(r) == hash(MaskCleanup(0.002, True, 200))
    assert r != MaskCleanup(min_area=0.002, keep_largest=True, max_hole=200, connectivity=4)


# ---------------------------------------------------------------- the oracle itself
def _same_partition(a, b):
    """Two labellings cut the same pixels into the same sets."""
    pairs = np.unique(np.stack([a.reshape(-1), b.reshape(-1)]), axis=1)
    return len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))


def test_oracle_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    full, cross = np.ones((3, 3), int), ndi.generate_binary_structure(2, 1)
    rng = np.random.default_rng(7)
    maps = [(rng.random((rng.integers(1, 40), rng.integers(1, 40))) < d).astype(np.uint8) for d in (0.3, 0.5, 0.62, 0.8) for _ in range(25)]
    maps += [m for hw in ((33, 65), (64, 64)) for m in O.patterns(*hw).values()] + [O.spiral(67)]
    for m in maps:
        for conn in (4, 8):
            lab, areas = O.label(m, conn)
            H, W = m.shape
            # canonical: a component's label is its first pixel, which labels itself; areas sit there and sum to the map
            idx = np.arange(H * W).reshape(H, W)
            assert (lab <= idx).all() and (lab.reshape(-1)[lab.reshape(-1)] == lab.reshape(-1)).all()
            assert areas.sum() == H * W and ((areas > 0) == (lab == idx)).all()
            fg_s, bg_s = (full, cross) if conn == 8 else (cross, full)
            for v in np.unique(m):
                sel = m == v
                ref, n = ndi.label(sel, structure=fg_s if v else bg_s)
                assert _same_partition(lab[sel], ref[sel]) and len(np.unique(lab[sel])) == n
            if set(np.unique(m)) <= {0, 1}:
                filled = O.clean(m, max_hole=2 ** 30, connectivity=conn)
                # (binary_fill_holes grows the background from the border: its structure is the BACKGROUND's connectivity)
                assert np.array_equal(filled.astype(bool), ndi.binary_fill_holes(m, structure=bg_s))


def test_oracle_known_answers():
    sp = O.spiral(67)
    lab, areas = O.label(sp, 4)
    assert int(sp.sum()) == 2311 and len(np.unique(lab)) == 2 and areas[0, 0] == 2311       # one component each, the long path
    cb = O.checkerboard(9, 11)
    assert int(cb.sum()) == 49
    assert np.array_equal(O.clean(cb, min_area=2, connectivity=8), cb) and not O.clean(cb, min_area=2, connectivity=4).any()
    m = np.zeros((7, 9), np.uint8)
    m[1:6, 1:8], m[3, 3], m[3, 5] = 2, 0, 0
    assert (O.clean(m, max_hole=1)[3, 2:7] == 2).all() and np.array_equal(O.clean(m, max_hole=0), m)
    two = np.zeros((5, 12), np.uint8)
    two[1:4, 1:4], two[1:4, 6:9] = 1, 1                                     # a tie: the first component wins
    kept = O.clean(two, keep_largest=True)
    assert kept[1:4, 1:4].all() and not kept[:, 5:].any()
    assert not O.clean(two, min_area=10, keep_largest=True).any()           # the survivor must pass min_area too
    assert np.array_equal(O.clean(two, min_area=0.15), two) and not O.clean(two, min_area=0.16).any()      # ceil(9.0) = 9, ceil(9.6) = 10


# ---------------------------------------------------------------- the C entry points without a device
@pytest.fixture(scope="module")
def L():
    from egm_unet_amd import build
    from egm_unet_amd._lib import lib
    build.build(verbose=False)
    return lib()


def test_abi_argument_checks_without_gpu(L):
    import ctypes
    c = L.cdll
    one = ctypes.c_void_p(16)                                               # never dereferenced: the checks run before any launch
    assert c.egm_ccl_workspace(1, 565, 753) > 565 * 753 * 9 and c.egm_ccl_workspace(2, 1, 1) > 0
    assert c.egm_ccl_workspace(1, 0, 5) == -1 and c.egm_ccl_workspace(1, 1 << 15, (1 << 15) + 1) == -1
    assert c.egm_ccl_workspace(1, 1 << 15, 1 << 15) > 0                     # exactly 2^30 pixels is admitted
    assert c.egm_ccl_label_u8(None, 1, 8, 8, 8, one, None, one, None) == -1 and b"null pointer" in c.egm_last_error()
    assert c.egm_ccl_label_u8(one, 1, 8, 8, 8, None, None, one, None) == -1 and b"null pointer" in c.egm_last_error()
    assert c.egm_ccl_label_u8(one, 1, 8, 8, 8, one, None, None, None) == -1 and b"null pointer" in c.egm_last_error()
    assert c.egm_ccl_label_u8(one, 1, 8, 8, 5, one, None, one, None) == -1 and b"connectivity 5" in c.egm_last_error()
    assert c.egm_ccl_label_u8(one, 1, 1 << 15, (1 << 15) + 1, 8, one, None, one, None) == -1 and b"2^30" in c.egm_last_error()
    assert c.egm_ccl_label_u8(one, 0, 8, 8, 8, one, None, one, None) == -1 and b"bad shape" in c.egm_last_error()
    clean = lambda *a: c.egm_mask_clean_u8(*a, None)                        # noqa: E731
    assert clean(None, 1, 8, 8, 8, one, one, one, None, None, None, None, 0, 0) == -1 and b"null pointer" in c.egm_last_error()
    assert clean(one, 1, 8, 8, 8, None, one, one, None, None, None, None, 0, 0) == -1 and b"null pointer" in c.egm_last_error()
    assert clean(one, 1, 8, 8, 8, one, one, None, None, None, None, None, 0, 0) == -1 and b"null pointer" in c.egm_last_error()
    assert clean(one, 1, 8, 8, 8, one, one, None, None, None, None, one, 4, 4) == -1 and b"yidx" in c.egm_last_error()
    assert clean(one, 1, 8, 8, 5, one, one, one, None, None, None, None, 0, 0) == -1 and b"connectivity 5" in c.egm_last_error()
    assert clean(one, 1, (1 << 15) + 1, 1 << 15, 4, one, one, one, None, None, None, None, 0, 0) == -1 and b"2^30" in c.egm_last_error()
    assert clean(one, 1, 8, 8, 4, one, one, None, one, one, None, one, 0, 4) == -1 and b"output shape" in c.egm_last_error()


# ---------------------------------------------------------------- the union-find core on the CPU
def test_host_check_program_builds_and_passes(tmp_path):
    """tools/ccl_host_check.cpp runs csrc/ccl_core.h -- the code the kernels run -- in the kernels' pass structure and in three pixel
    orders over the patterns, against a breadth-first reference.  Built with the address and undefined-behaviour sanitizers where the
    compiler has them (a plain host program: nothing is preloaded)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe, src = str(tmp_path / "ccl_host_check"), os.path.join(ROOT, "tools", "ccl_host_check.cpp")
    base = [cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", src, "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # the sanitizer runtimes linked into the program itself where the compiler can (then nothing depends on the order of shared
    # libraries in the process), otherwise as shared libraries, otherwise a plain build
    run = None
    for extra in (san + ["-static-libasan", "-static-libubsan"], san + ["-static-libsan"], san, []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode != 0:
            assert extra, r.stderr                                          # the plain build must compile
            continue
        run = subprocess.run([exe], capture_output=True, text=True)
        if run.returncode != 0 and extra and "runtime does not come first" in run.stderr:
            continue                                                        # a shared sanitizer runtime behind another preloaded library
        break
    assert run is not None and run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "ccl_host_check: ok" in run.stdout and "MISMATCH" not in run.stdout
    assert "spiral: 2311 foreground pixels, 1 foreground and 1 background components" in run.stdout
