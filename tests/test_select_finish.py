"""How a selection ends (csrc/select.hpp: block_select2_each): the candidates of the deciding bucket are ranked by counting up to SEL_RANK_MAX of
them and sorted by the bitonic network above, and the histogram of a level is zeroed by the bucket search that reads it, not cleared in front of
the next level.  The result is an exact order statistic either way, so everything here is bit for bit: the selections against NumPy
(kernel_refs.select_ref), the fits against what the build before this change returned for the same inputs (SHA-256, recorded with
tests/diag/select_finish_fit_hashes.py).

The selection inputs pin the number m of candidates: a plane of 2048 pixels whose wanted rank lies in a run of m keys that fills part of ONE
first-level bucket (the run starts on a bucket boundary counted from the plane's smallest key), everything else far below or far above.  m is
worked out again in the test from the keys, the way the kernel does."""
import hashlib

import numpy as np
import pytest

import kernel_refs as R
import test_fit_window as FW
import test_kernels_direct as D
import test_select_resident as S

pytestmark = pytest.mark.gpu

P = 2048                                # the smallest resident instance (16 slots per thread); variant 3 forces the streaming kernel at the same size
SEL_BITS, SEL_CAND, SEL_RANK_MAX = 13, 1024, 256        # select.hpp
MS = [1, 2, 3, 4, 5, 63, 64, 65, SEL_RANK_MAX - 1, SEL_RANK_MAX, SEL_RANK_MAX + 1, 1024, 1025]
REQS = [R.MEDIAN, 50.0, 75.0, 100.0]    # two selections of the same rank back to back, a third elsewhere, a plan that is done at once (k + 1 >= n)
SPAN = 0x10000000                       # far values: this many keys below / above the run; the key range is 2^29, so a first-level bucket is 2^17 keys
RUN_POS = 0xC0000000                    # key of 2.0f: a run of positive floats
RUN_ZERO = 0x7FFFFFFF                   # key of -0.0f; +0.0f is the next key


def sel_shift(lo, hi):
    bits = int(hi - lo).bit_length()
    return max(bits - SEL_BITS, 0)


def target_rank(n, q):
    if q is R.MEDIAN:
        return (n - 1) // 2 if n & 1 else n // 2 - 1
    return int(np.floor(np.float32(n - 1) * R.request_value(q)))


def frame(run_keys, n, k, pos, rng):
    """(values [P], mask [P]): n valid pixels whose sorted keys hold run_keys (sorted, len m) at ranks k - pos .. k - pos + m - 1; the plane's smallest
    key lies a whole number of first-level buckets below the run"""
    m = len(run_keys)
    lows, highs = k - pos, n - m - (k - pos)
    assert lows >= 0 and highs >= 1, (n, m, k, pos)
    base = int(run_keys[0])
    lo_keys = np.concatenate([[base - SPAN], base - SPAN + rng.integers(0, 1 << 20, max(lows - 1, 0))])[:lows]
    hi_keys = np.concatenate([[base + SPAN], base + SPAN - rng.integers(0, 1 << 20, highs - 1)])
    keys = np.concatenate([lo_keys, run_keys, hi_keys]).astype(np.uint32)
    vals = np.full(P, np.float32(3.0e38))                           # the pixels outside the mask: a value above everything
    idx = rng.permutation(P)[:n]
    vals[idx] = R.key2f(keys[rng.permutation(n)])
    mask = np.zeros(P, np.uint8)
    mask[idx] = 1
    return vals.astype(np.float32), mask


def candidates_of(vals, mask, k):
    """the count of the first-level bucket that holds rank k, as block_select2_each finds it"""
    keys = np.sort(R.f2key(R.select_compact(vals, mask))).astype(np.int64)
    lo, hi = int(keys[0]), int(keys[-1])
    sh = sel_shift(lo, hi)
    assert sh > 0
    return int((((keys - lo) >> sh) == ((keys[k] - lo) >> sh)).sum())


def runs(m, kind, base, pos):
    """sorted run of m keys from `base` on; pos: the wanted rank inside it"""
    r = base + np.arange(m, dtype=np.int64)
    if kind.startswith("dup"):                                      # the wanted rank at the start of, inside, at the end of a run of duplicates
        d = min(5, m)
        s = {"dup_start": pos, "dup_inside": pos - d // 2, "dup_end": pos - d + 1}[kind]
        s = min(max(s, 0), m - d)
        r[s:s + d] = r[s]
    elif kind == "one_key":
        r[:] = base + 7
    elif kind == "zeros":                                           # -0.0 and +0.0 only, the wanted rank next to where they meet when it can be
        r[:] = base + 1
        r[:min(max(pos, 1), m - 1) if m > 1 else 0] = base
    return r


def launch_cases(m, n):
    """[(kind, [frame0, frame1, frame2])]: the wanted rank first, in the middle and last in the bucket (last: rank + 1 is outside it, the neighbour
    sweep runs).  Frames 0 and 1 are built around the median's rank, frame 2 around the 75th percentile's, which leaves room below the run at every m."""
    km, k75 = target_rank(n, R.MEDIAN), target_rank(n, 75.0)
    assert target_rank(n, 50.0) == km
    out = []
    for kind in ("distinct", "dup_start", "dup_inside", "dup_end", "one_key", "zeros"):
        rng = np.random.default_rng(1000 * m + n + len(kind))
        frames = []
        for which, (k, want_pos) in enumerate(((km, 0), (km, m // 2), (k75, m - 1))):
            pos = min(max(want_pos, m + k + 1 - n), min(m - 1, k))
            base = RUN_ZERO if kind == "zeros" else RUN_POS
            v, mk = frame(runs(m, kind, base, pos), n, k, pos, rng)
            assert candidates_of(v, mk, k) == m, (m, kind, which)
            frames.append((v, mk))
        out.append((kind, frames))
    return out


@pytest.mark.parametrize("variant", [1, 3])
@pytest.mark.parametrize("m", MS)
def test_selection_with_m_candidates(pkg, m, variant):
    for n in (P, P - 1):                                            # medians of an even and an odd count
        for kind, frames in launch_cases(m, n):
            vals, mask = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
            got, cnt = D.gpu_select(pkg, vals, mask, P, None, False, REQS, variant)
            for b in range(3):
                exp, nn, nbrs = R.select_ref(vals[b], mask[b], REQS)
                assert cnt[b] == nn == n
                for j in range(len(REQS)):
                    assert R.same_result(got[b, j], exp[j]), (m, n, kind, b, REQS[j], hex(int(R.bits(got[b, j]).ravel()[0])), hex(int(R.bits(exp[j]).ravel()[0])), nbrs[j])


def test_chained_selections_share_one_histogram(pkg):
    """the chained hook: four selections in one launch, each over the elements not above the one before -- a histogram that the first left dirty
    shows in the second"""
    frames = [f for m in (5, 64, SEL_RANK_MAX + 1) for f in launch_cases(m, P)[0][1][:1]]
    vals, mask = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    reqs = [92.0, 50.0, 8.0, R.MEDIAN]
    got, cnt, inst = S.gpu_select_chained(pkg, vals, mask, False, reqs)
    for b in range(len(frames)):
        thr = None
        for j, q in enumerate(reqs):
            exp, _, _ = R.select_ref(vals[b], mask[b], [q], le_thr=thr)
            assert R.same_result(got[j, b], exp[0]), (b, j, got[j, b], exp[0])
            thr = exp[0]


# ---- fits: the medians' buckets full of duplicates, against the build before this change
FIT_SHAPES = [(32, 32), (64, 64), (224, 224)]
# recorded with tests/diag/select_finish_fit_hashes.py on the parent commit of this change
PARENT_SHA = {
    "32x32 plain order 1 col16": "9acba047d6bdee7b92fef8abc19ff36f6c9e258840fdf2688e6e911c0fc19316",
    "32x32 plain order 2 col16": "2c46f10b131da0e89a57f49540e299ad1af41f4d3c8f244e4349f014edf41603",
    "32x32 chain col16": "99c87ca707b856583046e318959be271a7d764bdb9a202d38c26ad4dff6dcf0a",
    "64x64 plain order 1 col16": "b086d65d5d55040beba76d238d9069f9ac4356ec78474ab6e0204c9a206681c9",
    "64x64 plain order 2 col16": "6c4db80eceff45a9a084e807f4123a5b0324950ec0ef50c9f1e8f4785d889ed3",
    "64x64 chain col16": "062a175c547de87d5362fd9ec026fd89aeabe7fbdbfb5fdbed3c2fad6991955e",
    "224x224 plain order 1 col56_g4": "281b6c2ed65564ad4784b5bfbb990f7f20619492077982ee40229cbceedd2d2d",
    "224x224 plain order 2 col56_g4": "4ee143779a6890b93d468200dcc38aa9d5d36c1eeefec75f14daf06d38313df4",
    "224x224 chain win48_g4": "f87b787153f232d2d5a6c7d2dc2908adb823da8a418a9eeff76d5cd1405616d9",
}


def fit_inputs(h, w):
    """B = 2: a constant plane and a plane quantised to 1/64, exact in float32 on 70 % of the pixels, with noise and gross outliers on the rest; a disc
    mask with a hole.  Meant to put many equal residuals around the medians (the quantised plane's residuals are tied wherever the fit rounds alike);
    how many are tied at the median is not asserted here -- the noisy 30 % perturb the fit -- and nothing below depends on it: the check is the
    parent's bits on these inputs, whatever their buckets hold.  The pinned duplicate cases are the selections' above."""
    yy, xx = np.indices((h, w))
    xn, yn = (xx - (w - 1) / 2) / ((w - 1) / 2), (yy - (h - 1) / 2) / ((h - 1) / 2)
    zs, ms = [], []
    for i in range(2):
        rng = np.random.default_rng(7 * h + w + i)
        z = np.full((h, w), 1.5) if i == 0 else np.round((1.0 + 0.5 * xn - 0.25 * yn) * 64) / 64
        noisy = rng.random((h, w)) < 0.3
        z = z + noisy * (0.02 * rng.standard_normal((h, w)) + (rng.random((h, w)) < 0.1) * rng.uniform(-4, 4, (h, w)))
        m = (xn ** 2 + yn ** 2 <= 1.0) & ((xn - 0.3) ** 2 + (yn + 0.2) ** 2 > 0.02)
        zs.append(z.astype(np.float32))
        ms.append(m.astype(np.uint8))
    return np.stack(zs), np.stack(ms)


def fit_hashes(pkg, h, w):
    """{case: sha256} of what the plain fit (orders 1 and 2) and the chained launch (order 1 then 2) return"""
    z, m = fit_inputs(h, w)
    out = {}

    def sha(*arrays):
        hh = hashlib.sha256()
        for a in arrays:
            hh.update(np.ascontiguousarray(a).tobytes())
        return hh.hexdigest()

    for order in (1, 2):
        coef, resid, inst = D.gpu_polyfit(pkg, z, m, order, 0)
        out["%dx%d plain order %d %s" % (h, w, order, inst)] = sha(coef, resid)
    inst, coef, r1, r2, need = FW.chain(pkg, z, m, (1, 2), (0, 0), 0)
    out["%dx%d chain %s" % (h, w, inst)] = sha(coef, r1, r2, need)
    return out


@pytest.mark.parametrize("shape", FIT_SHAPES)
def test_fits_return_the_parents_bits(pkg, shape):
    got = fit_hashes(pkg, *shape)
    exp = {k: v for k, v in PARENT_SHA.items() if k.startswith("%dx%d " % shape)}
    assert len(exp) == 3 and got == exp
