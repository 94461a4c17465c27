"""The binary dilate / erode kernels launched directly (csrc/test_hooks.h: vistaf_ftp_test_morph), each of launch_morph's three kernels forced
and as dispatched, against the brute force of tests/morph_cases.py: exact, outputs strictly 0 / 1.  Every test asserts the kernel the hook
reports.  A CPU test holds the brute force against the oracle's own restatement (oracle/cvlite.py dilate / erode), so the two pin each other."""
import ctypes

import numpy as np
import pytest

import morph_cases as C
from oracle import cvlite

E_INVALID = -1
_REF = {}


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()               # a copy: the shared stacks are read-only


def _ptr(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + offset) if t is not None else None


def _stack(h, w):
    """(names, masks [n, h, w]) of the catalogue, n a multiple of 3 (filled up from the front); shared, never written to"""
    if (h, w) not in _REF:
        cat = C.masks(h, w)
        names = list(cat)
        names += names[:(-len(names)) % 3]
        st = np.stack([cat[k] for k in names])
        st.setflags(write=False)
        _REF[(h, w)] = (names, st)
    return _REF[(h, w)]


def _ref(h, w, e, dilate):
    key = (h, w, e, dilate)
    if key not in _REF:
        r = C.morph_ref(_stack(h, w)[1], C.element(e), dilate)
        r.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def _first_diff(got, want, names=None):
    bad = np.argwhere(got != want)
    b = tuple(bad[0])
    return "%d pixels differ, first at %s%s: got %r, want %r" % (len(bad), b, " (%s)" % names[b[0]] if names else "", got[b], want[b])


# =======================================================================================================================================
# CPU: the reference itself

def test_elements_are_what_opencv_documents():
    """known answers of cv2.getStructuringElement, and the oracle's ellipse for every size"""
    assert C.ellipse(5).tolist() == [[0, 0, 1, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [0, 0, 1, 0, 0]]
    assert C.ellipse(3).tolist() == [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
    assert C.ellipse(2).tolist() == [[0, 1], [1, 1]] and C.ellipse(1).tolist() == [[1]]
    assert C.ellipse(4).tolist() == [[0, 0, 1, 0], [1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]]
    for k in C.ELLIPSES:
        assert np.array_equal(C.ellipse(k), cvlite.ellipse_se(k)), k
        assert C.symmetric(C.ellipse(k)) == (k % 2 == 1), k
    assert C.element((1, 4, 6)).shape == (7, 5) and C.element((1, 127, 33)).shape == (33, 127)
    assert all(C.symmetric(C.element(e)) for e in C.ELEMENTS if e[0] != 0)
    assert C.hourglass(5).tolist() == [[1, 1, 1, 1, 1], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0], [0, 1, 1, 1, 0], [1, 1, 1, 1, 1]]


def test_only_the_hourglass_sees_a_replicated_border():
    """Why the hook has an element no cv shape gives: with every ellipse and rectangle an erosion (or dilation) that read the nearest border
    pixel for a pixel outside the image gives the bits of the real operation, on every mask of the catalogue; with the hourglass it does not."""
    for h, w in ((9, 40), (33, 65)):
        st = _stack(h, w)[1]
        for e in C.ELEMENTS:
            same = all(np.array_equal(C.morph_ref(st, C.element(e), d), C.morph_ref(st, C.element(e), d, replicate=True)) for d in (0, 1))
            assert same == (e[0] != 2), (C.element_id(e), h, w)
        for k in C.HOURGLASSES if (h, w) == (33, 65) else ():           # the erosion on its own, where the frame is large enough for all three sizes
            assert not np.array_equal(C.morph_ref(st, C.hourglass(k), 0), C.morph_ref(st, C.hourglass(k), 0, replicate=True)), k


def _square(se):
    """an odd-sided element embedded in the square one the oracle's morphology takes: same anchor, same offsets"""
    ky, kx = se.shape
    k = max(ky, kx)
    if ky % 2 == 0 or kx % 2 == 0:
        assert ky == kx
        return se
    sq = np.zeros((k, k), np.uint8)
    sq[(k - ky) // 2:(k - ky) // 2 + ky, (k - kx) // 2:(k - kx) // 2 + kx] = se
    return sq


@pytest.mark.parametrize("e", C.ELEMENTS, ids=[C.element_id(e) for e in C.ELEMENTS])
def test_brute_force_equals_the_oracle_morphology(e):
    """every element on a few masks of two small frames: the NumPy brute force and oracle/cvlite.py agree, both operations"""
    se = C.element(e)
    for h, w in ((9, 40), (33, 65)):
        cat = C.masks(h, w)
        for name in ("zeros", "ones", "corners_and_mid_edges", "border", "checker", "random_0.02", "random_0.5", "random_0.98", "col_last_off"):
            m = cat[name]
            for dilate, fn in ((1, cvlite.dilate), (0, cvlite.erode)):
                want = (fn(m, _square(se), 1) != 0).astype(np.uint8)
                got = C.morph_ref(m, se, dilate)
                assert set(np.unique(got)) <= {0, 1} and np.array_equal(got, want), (name, h, w, dilate)


def test_catalogue_is_what_it_says():
    for h, w in C.SHAPES:
        names, st = _stack(h, w)
        assert st.dtype == np.uint8 and len(names) % 3 == 0 and {"zeros", "ones", "border", "checker", "random_0.5", "row_mid", "col_mid"} <= set(names)
        assert not st[names.index("zeros")].any() and st[names.index("ones")].all()
        assert set(np.unique(st)) == {0, 1, 2, 255}
        b = st[names.index("border")] != 0
        assert b[0].all() and b[-1].all() and b[:, 0].all() and b[:, -1].all() and int(b.sum()) == h * w - max(h - 2, 0) * max(w - 2, 0)
    # the tier rules restated: even ellipses are not symmetric, 127 columns still fit the word shift, a frame of 4097 words does not
    assert C.expected_tier(C.ellipse(4), 64, 64, C.BITS) is None and C.expected_tier(C.ellipse(5), 64, 64, C.DISPATCH) == C.BITS
    assert C.expected_tier(C.rect(127, 33), 40, 200, C.BITS) == C.BITS and C.expected_tier(C.ellipse(8), 64, 64, C.DISPATCH) == C.PREFIX
    assert C.expected_tier(C.ellipse(4), 64, 64, C.DISPATCH) == C.GENERIC and C.expected_tier(C.ellipse(8), 64, 64, C.DISPATCH_NO_SCRATCH) == C.GENERIC
    assert C.expected_tier(C.ellipse(13), 66, 4033, C.DISPATCH) == C.PREFIX and C.expected_tier(C.ellipse(13), 64, 4096, C.DISPATCH) == C.BITS


# =======================================================================================================================================
# GPU

def gpu_morph(pkg, d_src, d_out, B, h, w, e, dilate, tier, frame0=0, d_static=None, d_frame=None):
    """one call of the hook on frames frame0 .. frame0 + B of the device stacks; returns what the hook returns"""
    off = frame0 * h * w
    return pkg._lib.load().vistaf_ftp_test_morph(_ptr(d_src, off), _ptr(d_out, off), B, h, w, e[0], e[1], e[2], dilate, _ptr(d_static),
                                                 _ptr(d_frame, off), tier, None)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", C.SHAPES, ids=["%dx%d" % s for s in C.SHAPES])
def test_every_tier_equals_brute_force(pkg, h, w):
    """every element, both operations, the whole catalogue in batches of three different frames (and the last frame alone, B = 1): each kernel
    forced and both dispatches give the reference's bits and report the kernel the rules name; the bit-plane kernel refuses what it does not take"""
    import torch
    names, st = _stack(h, w)
    n = len(names)
    d_src = _dev(st)
    ran = set()
    for e in C.ELEMENTS:
        se = C.element(e)
        for dilate in (1, 0):
            want = _ref(h, w, e, dilate)
            for tier in (C.GENERIC, C.PREFIX, C.BITS, C.DISPATCH, C.DISPATCH_NO_SCRATCH):
                exp = C.expected_tier(se, h, w, tier)
                d_out = torch.full((n, h, w), 7, dtype=torch.uint8, device="cuda")
                if exp is None:
                    assert gpu_morph(pkg, d_src, d_out, 3, h, w, e, dilate, tier) == E_INVALID, (C.element_id(e), tier)
                    assert bool((d_out == 7).all())
                    continue
                for f0 in range(0, n - 3, 3):
                    assert gpu_morph(pkg, d_src, d_out, 3, h, w, e, dilate, tier, f0) == exp, (C.element_id(e), tier, pkg._lib.load().vistaf_ftp_last_error())
                for f0 in (n - 3, n - 2, n - 1):                                  # B = 1, frames at unaligned addresses when h * w is odd
                    assert gpu_morph(pkg, d_src, d_out, 1, h, w, e, dilate, tier, f0) == exp
                got = d_out.cpu().numpy()
                assert np.array_equal(got, want), (C.element_id(e), dilate, tier, _first_diff(got, want, names))
                ran.add(exp)
    assert ran == {C.GENERIC, C.PREFIX, C.BITS}


GATE_SHAPES = ((33, 65), (40, 200))
GATE_ELEMENTS = ((0, 5, 0), (0, 4, 0), (0, 8, 0), (1, 3, 31), (1, 127, 1), (2, 7, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", GATE_SHAPES, ids=["%dx%d" % s for s in GATE_SHAPES])
def test_gating_masks_on_every_tier(pkg, h, w):
    """and_static ([h, w], one for the batch) and and_frame ([B, h, w]) with values from {0, 1, 2, 255}: each absent, each present, both, all-zero"""
    import torch
    B = 3
    names, st = _stack(h, w)
    pick = [names.index(k) for k in ("random_0.5", "random_0.98", "border")]
    src = np.ascontiguousarray(st[pick])
    d_src = _dev(src)
    gates = C.gates(h, w, B, 31 * h + w)
    assert set(np.unique(gates["both"][0])) == {0, 1, 2, 255} and not gates["static_zero"][0].any()
    for e in GATE_ELEMENTS:
        se = C.element(e)
        for dilate in (1, 0):
            base = _ref(h, w, e, dilate)[pick]
            assert base.any()
            for gname, (gs, gf) in gates.items():
                want = base.copy()
                if gs is not None:
                    want &= (gs != 0)[None]
                if gf is not None:
                    want &= gf != 0
                d_s, d_f = (None if g is None else _dev(g) for g in (gs, gf))
                for tier in (C.GENERIC, C.PREFIX, C.BITS):
                    exp = C.expected_tier(se, h, w, tier)
                    if exp is None:
                        continue
                    d_out = torch.full((B, h, w), 7, dtype=torch.uint8, device="cuda")
                    assert gpu_morph(pkg, d_src, d_out, B, h, w, e, dilate, tier, 0, d_s, d_f) == exp
                    got = d_out.cpu().numpy()
                    assert np.array_equal(got, want), (C.element_id(e), dilate, gname, tier, _first_diff(got, want))


# the smallest frames that leave the bit-plane kernel, h * ceil(w / 64) > 4096, one wide and one tall
NATURAL_SHAPES = ((66, 4033), (4100, 60))
NATURAL_ELEMENTS = (((0, 13, 0), C.PREFIX), ((1, 3, 31), C.PREFIX), ((0, 3, 0), C.GENERIC), ((1, 3, 3), C.GENERIC))


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", NATURAL_SHAPES, ids=["%dx%d" % s for s in NATURAL_SHAPES])
def test_natural_dispatch_beyond_the_bit_planes(pkg, h, w):
    """B = 2 frames as a session would hand them over: with scratch the tall elements take the row-prefix kernels and the short ones k_morph,
    without scratch (the k_inpaint_cl.hip call) everything takes k_morph.  Row 7 of frame 0 is all ones: its uint16 counts pass 255 and 4032."""
    import torch
    rng = np.random.default_rng(h + w)
    vals = np.array([1, 2, 255], np.uint8)[rng.integers(0, 3, (2, h, w))]
    src = np.stack([rng.random((h, w)) < 0.002, rng.random((h, w)) < 0.998])      # sparse: the dilations say something; dense: the erosions do
    src[0, 7, :] = True
    src[1, :, w // 2] = True
    src[1, h // 2, :] = False
    src = (src * vals).astype(np.uint8)
    d_src = _dev(src)
    assert h * ((w + 63) // 64) > 4096
    for e, with_scratch in NATURAL_ELEMENTS:
        se = C.element(e)
        assert C.expected_tier(se, h, w, C.DISPATCH) == with_scratch and C.expected_tier(se, h, w, C.BITS) is None
        for dilate in (1, 0):
            want = C.morph_ref(src, se, dilate)
            assert 0 < int(want.sum()) < want.size
            for tier, exp in ((C.DISPATCH, with_scratch), (C.DISPATCH_NO_SCRATCH, C.GENERIC)):
                d_out = torch.full((2, h, w), 7, dtype=torch.uint8, device="cuda")
                assert gpu_morph(pkg, d_src, d_out, 2, h, w, e, dilate, tier) == exp, (C.element_id(e), tier)
                got = d_out.cpu().numpy()
                assert np.array_equal(got, want), (C.element_id(e), dilate, tier, _first_diff(got, want))
            d_out = torch.full((2, h, w), 7, dtype=torch.uint8, device="cuda")
            assert gpu_morph(pkg, d_src, d_out, 2, h, w, e, dilate, C.BITS) == E_INVALID and bool((d_out == 7).all())


@pytest.mark.gpu
def test_refused_arguments(pkg):
    import torch
    lib = pkg._lib.load()
    h, w = 8, 70
    a = torch.zeros((2, h, w), dtype=torch.uint8, device="cuda")
    o = torch.full((2, h, w), 7, dtype=torch.uint8, device="cuda")
    pa, po = _ptr(a), _ptr(o)
    ok = dict(src=pa, dst=po, B=2, h=h, w=w, shape=1, kx=3, ky=3, dilate=1, st=None, fr=None, tier=0)
    bad = [dict(src=None), dict(dst=None), dict(dst=pa), dict(B=0), dict(h=0), dict(w=0), dict(B=-1), dict(kx=128), dict(kx=0), dict(ky=34), dict(ky=0),
           dict(shape=0, kx=34), dict(shape=0, kx=0), dict(shape=3), dict(shape=-1), dict(tier=5), dict(tier=-1),
           dict(shape=2, kx=4), dict(shape=2, kx=1), dict(shape=2, kx=35),
           dict(tier=3, shape=0, kx=4),                       # an element that is not symmetric about its anchor
           dict(tier=3, shape=0, kx=2)]
    for b in bad:
        c = dict(ok, **b)
        rc = lib.vistaf_ftp_test_morph(c["src"], c["dst"], c["B"], c["h"], c["w"], c["shape"], c["kx"], c["ky"], c["dilate"], c["st"], c["fr"], c["tier"], None)
        assert rc == E_INVALID, b
        assert lib.vistaf_ftp_last_error()
    assert bool((o == 7).all())
    # a frame of 4097 words: refused by the bit-plane kernel before anything is read (the planes are far smaller than such a frame)
    assert lib.vistaf_ftp_test_morph(pa, po, 1, 4097, 1, 1, 3, 3, 1, None, None, 3, None) == E_INVALID
    assert lib.vistaf_ftp_test_morph(pa, po, 1, 1, 65536, 1, 3, 3, 1, None, None, 2, None) == E_INVALID       # uint16 row counts
    c = ok
    assert lib.vistaf_ftp_test_morph(c["src"], c["dst"], 2, h, w, 1, 127, 33, 1, None, None, 0, None) == C.BITS and not bool(o.any())
