"""Inputs for tests/test_dft_direct.py: magnitude planes for the peak search and hand-built peak lists for the carrier choice, each with the
properties its name promises.  tests/test_kernel_refs.py asserts those properties on the CPU; nothing here touches the GPU."""
import collections

import numpy as np

import kernel_refs as R

TP_L, TP_THREADS = 4, 1024          # k_top_peaks: elements every thread keeps, threads of its one workgroup

PeakCase = collections.namedtuple("PeakCase", "name mag dc npeaks distinct overflow")
CarrierCase = collections.namedtuple("CarrierCase", "name peaks mag bw frac exact_half")


# ---------------------------------------------------------------------------------------------------------------------------------------
# peak search

def _distinct_plane(rng, shape):
    """positive, pairwise distinct float64 values in random order"""
    n = int(np.prod(shape))
    return rng.permutation(1.0 + np.arange(n) / n + rng.random() * 1e-3).reshape(shape)


def peak_cases():
    rng = np.random.default_rng(20240)
    out = []

    def add(name, mag, dc, npeaks, distinct=True, overflow=False):
        mag = np.asarray(mag, np.float64)
        out.append(PeakCase(name, mag if mag.ndim == 3 else mag[None], dc, npeaks, distinct, overflow))

    add("plane_of_64_all_listed", _distinct_plane(rng, (8, 8)), 0, 64)
    add("40x64", _distinct_plane(rng, (40, 64)), 3, 12)
    add("130x129_64_peaks", _distinct_plane(rng, (130, 129)), 10, 64)
    add("dc_box_is_the_plane", _distinct_plane(rng, (40, 64)), 40, 12, distinct=False)
    add("batch_of_3", np.stack([_distinct_plane(rng, (40, 64)) for _ in range(3)]), 2, 10)
    # the fallback: more of the result than a thread keeps in one thread's stride.  A stride of a 128 x 64 plane holds eight elements, so
    # that plane carries the eight largest at indices = 5 mod 1024 and the next four at indices = 6 mod 1024; all twelve in one stride
    # take 128 x 96, where a stride holds twelve
    m = 0.5 * _distinct_plane(rng, (128, 64))
    m.ravel()[5 + 1024 * np.arange(8)] = 10.0 + rng.permutation(8)
    m.ravel()[6 + 1024 * np.arange(2, 6)] = 5.0 + rng.permutation(4)
    add("crowded_128x64", m, 4, 12, overflow=True)
    m = 0.5 * _distinct_plane(rng, (128, 96))
    m.ravel()[5 + 1024 * np.arange(12)] = 10.0 + rng.permutation(12)
    add("crowded_128x96_twelve_in_one_stride", m, 4, 12, overflow=True)
    # ties: a plateau of six equal maxima, five of them in one thread's stride
    m = 0.5 * _distinct_plane(rng, (128, 64))
    m.ravel()[[7 + 1024 * 6, 7 + 1024 * 1, 7 + 1024 * 4, 7 + 1024 * 2, 7 + 1024 * 7, 300]] = 3.0
    add("plateau_of_6", m, 4, 12, distinct=False, overflow=True)
    # fewer positive values than peaks, all in thread 0's stride: the N-th result is a zero
    m = np.zeros((128, 64))
    m.ravel()[1024 * np.arange(8)] = 1.0 + np.arange(8)
    add("sparse_8_positive", m, 4, 12, distinct=False, overflow=True)
    add("all_zero", np.zeros((128, 64)), 4, 12, distinct=False)
    return out


def overflows(mag, dc, npeaks):
    """does some thread of k_top_peaks hold more than TP_L of the result (by the kernel's rule), so that its one pass cannot be enough"""
    w = mag.shape[1]
    idx = np.array([y * w + x for x, y, _ in R.top_peaks_rule(mag, dc, npeaks)])
    return int(np.bincount(idx % TP_THREADS).max()) > TP_L


# ---------------------------------------------------------------------------------------------------------------------------------------
# carrier choice

HF, WF = 40, 48                     # centre row 20, centre column 24
HALF = 1.0 - 1e-12                  # the double m with m + 1e-12 == 1.0: log(m + 1e-12) is exactly 0


def _plane(rng):
    return rng.uniform(0.5, 2.0, (HF, WF))


def _bump(mag, x, y, left=0.6, right=0.5, up=0.55, down=0.7, top=3.0):
    """a local maximum at (x, y) with the given neighbours (as fractions of its value)"""
    mag[y, x] = top
    for dx, dy, f in ((-1, 0, left), (1, 0, right), (0, -1, up), (0, 1, down)):
        if 0 <= y + dy < mag.shape[0] and 0 <= x + dx < mag.shape[1]:
            mag[y + dy, x + dx] = top * f
    return mag


def carrier_cases():
    rng = np.random.default_rng(77)
    out = []

    def add(name, peaks, mag, bw=3, frac=0.12, exact_half=False):
        out.append(CarrierCase(name, [(int(x), int(y), float(v)) for x, y, v in peaks], np.asarray(mag, np.float64), bw, frac, exact_half))

    # filters
    add("no_peak_right_of_centre", [(10, 20, 5.0), (24, 22, 4.0), (3, 30, 3.0)], _bump(_plane(rng), 10, 20))
    add("no_peak_near_the_centre_row", [(30, 5, 5.0), (33, 30, 6.0), (12, 36, 7.0)], _bump(_plane(rng), 33, 30))
    add("both_filters_strongest_left_next_far", [(10, 20, 9.0), (30, 33, 8.0), (31, 22, 7.0), (35, 19, 6.0)], _bump(_plane(rng), 31, 22))
    add("both_filters_strongest_right_but_far", [(30, 33, 9.0), (10, 20, 8.0), (31, 17, 7.0)], _bump(_plane(rng), 31, 17))
    add("equal_values_first_listed_wins", [(10, 20, 9.0), (33, 21, 7.0), (29, 19, 7.0), (36, 20, 7.0)], _bump(_bump(_plane(rng), 33, 21), 29, 19))
    add("one_peak", [(31, 21, 2.0)], _bump(_plane(rng), 31, 21))
    pos = rng.permutation(HF * WF)[:64]
    pk64 = [(p % WF, p // WF, 64.0 - i) for i, p in enumerate(pos)]
    ch = R.O.choose_carrier_peak(pk64, HF, WF, 0.12)
    m = _plane(rng)
    if 0 < ch[0] < WF - 1 and 0 < ch[1] < HF - 1:
        _bump(m, ch[0], ch[1])
    add("64_peaks", pk64, m)
    # max_dy = int(0.12 * 40) = int(4.8) = 4: a stronger peak five rows off is rejected, the one four rows off taken
    add("max_dy_truncates", [(30, 25, 9.0), (32, 24, 8.0)], _bump(_plane(rng), 32, 24))
    # no refinement on a border
    for name, x, y in (("border_left", 0, 20), ("border_right", WF - 1, 20), ("border_top", 30, 0), ("border_bottom", 30, HF - 1)):
        add(name, [(x, y, 4.0)], _plane(rng))
    # the parabola's special cases
    m = _bump(_plane(rng), 31, 21)
    m[21, 30] = m[21, 32] = m[21, 31]
    add("three_equal_neighbours_in_x", [(31, 21, 3.0)], m)
    add("zero_magnitude_neighbour", [(31, 21, 3.0)], _bump(_plane(rng), 31, 21, left=0.0))
    add("offsets_below_1e-6_both_zeroed", [(31, 21, 3.0)], _bump(_plane(rng), 31, 21, left=0.5, right=0.5 * (1 + 1e-7), up=0.6 * (1 - 1e-7), down=0.6))
    add("offset_below_1e-6_in_x_only_both_kept", [(31, 21, 3.0)], _bump(_plane(rng), 31, 21, left=0.5, right=0.5 * (1 + 1e-7)))
    # an exact half: log(f0) = log(f+1) = 0 exactly, f-1 smaller, so the vertex is at +0.5 in x and in y; np.round goes to even
    for px in (20, 21):
        m = _plane(rng)
        m[21, px] = m[21, px + 1] = m[22, px] = HALF
        m[21, px - 1], m[20, px] = 0.25, 0.125
        add("exact_half_px_%d" % px, [(px, 21, 1.0)], m, exact_half=True)
    add("chosen_value_zero", [(31, 21, 0.0), (10, 20, 0.0)], _bump(_plane(rng), 31, 21))
    # patches clipped by the spectrum border (bw = 3 reaches past it), the peak itself one bin inside
    for name, x, y in (("clipped_left", 1, 20), ("clipped_right", WF - 2, 21), ("clipped_top", 30, 1), ("clipped_bottom", 31, HF - 2)):
        add(name, [(x, y, 4.0)], _bump(_plane(rng), x, y))
    return out
