"""Inputs and the NumPy restatement of the per-contact table for tests/test_contacts.py.

`synth.deformed_frame` draws one bump per frame; the frames here carry k = 1..4 Gaussian bumps so that a depth map holds several separate
contacts.  `numpy_contacts` is the definition of the table (include/vistaf_ftp.h, vistaf_ftp_contacts) written out in NumPy on a depth map and
a kept mask, with `oracle.cvlite.cc8` for the 8-connected components.
"""
import numpy as np

from oracle import cvlite

SEED0 = 1000 * 7
FIELDS = ("pixels", "contact_pixels", "contact_area_mm2", "volume_cm3", "max_depth_mm", "argmax_index", "centroid_x", "centroid_y", "force_N",
          "bbox_x0", "bbox_y0", "bbox_x1", "bbox_y1")
F = {name: i for i, name in enumerate(FIELDS)}


def bumps_phase(h, w, circle, k, rng, n_sigma):
    """-(sum of k Gaussians): centres on a ring of radius 0.5 R around the ROI centre at equal angles from a random start, amplitude
    U(0.6, 1.2) rad, sigma U(0.05, 0.08) * n_sigma each"""
    cx, cy, r = circle
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a0 = rng.uniform(0.0, 2.0 * np.pi)
    phi = np.zeros((h, w))
    for j in range(k):
        ang = a0 + 2.0 * np.pi * j / k
        x0, y0 = cx + 0.5 * r * np.cos(ang), cy + 0.5 * r * np.sin(ang)
        amp, sig = rng.uniform(0.6, 1.2), rng.uniform(0.05, 0.08) * n_sigma
        phi -= amp * np.exp(-((xx - x0) ** 2 + (yy - y0) ** 2) / (2.0 * sig * sig))
    return phi


def multi_contact_frame(pkg, n, index, period=None):
    """frame `index` of the multi-contact set at n x n: seed 1000 * 7 + index, k = 1 + index % 4 bumps"""
    rng = np.random.default_rng(SEED0 + index)
    phi = bumps_phase(n, n, pkg.synth.roi_circle(n), 1 + index % 4, rng, n)
    return pkg.synth._base(n, phi, rng, period)


def multi_contact_batch(pkg, n, start, count, period=None):
    return np.stack([multi_contact_frame(pkg, n, start + i, period) for i in range(count)])


def odd_size_frames(h, w, circle, period, count):
    """(reference, frames) at h x w with an off-centre ROI circle: the fringe model of tests/test_gpu_parity.py::test_non_square_odd_sizes
    with the multi-bump phase"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)

    def mk(phi, rng):
        img = 128.0 * (1.0 + 0.1 * np.cos(xx / 60.0)) * (0.55 + 0.35 * np.cos(2 * np.pi * xx / period + phi)) + rng.normal(0, 2.0, (h, w))
        return np.clip(np.rint(img), 0, 255).astype(np.uint8)

    ref = mk(0.0, np.random.default_rng(SEED0 + 999))
    frames = []
    for i in range(count):
        rng = np.random.default_rng(SEED0 + 100 + i)
        frames.append(mk(bumps_phase(h, w, circle, 1 + i % 4, rng, min(h, w)), rng))
    return ref, np.stack(frames)


def numpy_contacts(depth_mm, kept, mm_per_px, eps, force_fn):
    """The table of one frame, ALL contacts, in the table's order.  depth_mm: float32 map (NaN counts as 0); kept: bool mask.
    Returns (rows [count, 13] float64, labels_in_order) where labels_in_order[k] is the boolean mask of contact k."""
    d = np.nan_to_num(np.asarray(depth_mm, dtype=np.float32), nan=0.0)
    h, w = d.shape
    kept = np.asarray(kept, dtype=bool)
    _, labels, _ = cvlite.cc8(kept.astype(np.uint8))
    flat_d, flat_l = d.ravel(), labels.ravel()
    area_px = float(mm_per_px) * float(mm_per_px)
    recs = []
    for lab in np.unique(flat_l[kept.ravel()]):
        idx = np.flatnonzero(flat_l == lab)                  # row-major, ascending
        dv = flat_d[idx]
        j = int(np.argmax(dv))                               # first occurrence of the maximum
        c = dv > np.float32(eps)
        ys, xs = idx // w, idx % w
        dc = dv[c].astype(np.float64)
        vol32 = float(np.float32(dc.sum()))
        n_c = int(c.sum())
        volume = vol32 * area_px / 1000.0 if n_c else 0.0
        row = np.full(len(FIELDS), np.nan)
        row[F["pixels"]] = idx.size
        row[F["contact_pixels"]] = n_c
        row[F["contact_area_mm2"]] = float(n_c) * area_px
        row[F["volume_cm3"]] = volume
        row[F["max_depth_mm"]] = float(dv[j])
        row[F["argmax_index"]] = int(idx[j])
        if n_c:
            row[F["centroid_x"]] = float((xs[c].astype(np.float64) * dc).sum() / dc.sum())
            row[F["centroid_y"]] = float((ys[c].astype(np.float64) * dc).sum() / dc.sum())
        row[F["force_N"]] = force_fn(volume)
        row[F["bbox_x0"]], row[F["bbox_y0"]], row[F["bbox_x1"]], row[F["bbox_y1"]] = xs.min(), ys.min(), xs.max(), ys.max()
        recs.append((row, labels == lab))
    recs.sort(key=lambda t: (-t[0][F["max_depth_mm"]], t[0][F["argmax_index"]]))
    rows = np.stack([t[0] for t in recs]) if recs else np.zeros((0, len(FIELDS)))
    return rows, [t[1] for t in recs]


def numpy_index_plane(masks, shape, k):
    plane = np.full(shape, -1, np.int8)
    for i, m in enumerate(masks[:k]):
        plane[m] = i
    return plane
