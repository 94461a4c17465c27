"""Regenerate tests/golden/tempmodel_fixture.npz: scikit-learn temperature pipelines fitted on synthetic Lab-like data, exported as
TempModel JSON, with input rows and scikit-learn's own predictions for float32 and float64 rows.

Needs scikit-learn (the package itself does not).  Run from the repository root:  python tests/golden/make_tempmodel_fixture.py
The fixture lets the GPU tests compare against scikit-learn without it being installed where they run.
"""
import importlib
import json
import os
import sys

import numpy as np
from sklearn.isotonic import IsotonicRegression
from sklearn.linear_model import HuberRegressor
from sklearn.pipeline import make_pipeline
from sklearn.preprocessing import PolynomialFeatures, StandardScaler

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
TM = importlib.import_module("vistaf-roboskin-vision-integrated-multimodal-sensor_amd.tempmodel")
OUT = os.path.join(ROOT, "tests", "golden", "tempmodel_fixture.npz")
LAB, LABG = ("L", "a", "b"), ("L", "a", "b", "gray")

# name, features, degree, huber alpha, scaler with_mean, include_bias, isotonic ("clip" / "nan" / "k1" / None)
SPECS = [
    ("lab_d1_clip", LAB, 1, 1e-6, True, True, "clip"),
    ("lab_d2_nan", LAB, 2, 1e-6, True, True, "nan"),
    ("lab_d3", LAB, 3, 1e-6, True, True, None),
    ("lab_d4_k1", LAB, 4, 1e-6, True, True, "k1"),
    ("labg_d1", LABG, 1, 1e-4, True, True, None),
    ("labg_d2_nomean", LABG, 2, 1e-4, False, True, "clip"),
    ("labg_d3_nobias", LABG, 3, 1e-4, True, False, None),
    ("labg_d4", LABG, 4, 1e-4, True, True, "nan"),
]


def synthetic_lab(rng, n, lo=0.0, hi=255.0):
    """Lab-like rows (L, a, b, gray on 0..255) with gray tied to L, and a smooth temperature in 20..60 degC"""
    L = rng.uniform(lo, hi, n)
    a = 128 + rng.uniform(lo - 128, hi - 128, n) * 0.6
    b = 128 + rng.uniform(lo - 128, hi - 128, n) * 0.6
    gray = np.clip(0.9 * L + rng.normal(0, 8, n), 0, 255)
    X = np.stack([L, a, b, gray], 1)
    t = 40 + 0.08 * (L - 128) - 0.05 * (a - 128) + 0.03 * (b - 128) + 2e-4 * (L - 128) * (a - 128) - 0.02 * (gray - L)
    return X, t + rng.normal(0, 0.4, n)


def main():
    rng = np.random.default_rng(20261016)
    Xtr, ytr = synthetic_lab(rng, 3000, 20.0, 235.0)
    Xte, _ = synthetic_lab(rng, 512)                       # wider than the training range: the "nan" calibrators leave their range
    Xte = np.round(Xte, 2)
    models, pred32, pred64 = {}, {}, {}
    for name, feats, deg, alpha, with_mean, bias, iso_kind in SPECS:
        cols = [LABG.index(f) for f in feats]
        pipe = make_pipeline(StandardScaler(with_mean=with_mean), PolynomialFeatures(deg, include_bias=bias),
                             HuberRegressor(epsilon=1.2, alpha=alpha, max_iter=10000)).fit(Xtr[:, cols], ytr)
        iso = None
        if iso_kind == "k1":
            iso = IsotonicRegression(out_of_bounds="clip").fit(np.full(8, 31.0), np.linspace(25, 35, 8))
        elif iso_kind is not None:
            p = pipe.predict(Xtr[:, cols])
            keep = (p > np.percentile(p, 10)) & (p < np.percentile(p, 90)) if iso_kind == "nan" else slice(None)
            iso = IsotonicRegression(out_of_bounds=iso_kind).fit(p[keep], ytr[keep])
        m = TM.TempModel.from_sklearn(pipe, iso, features=feats)
        models[name] = m.to_dict()

        def run(X):
            y = pipe.predict(X)
            return iso.predict(y) if iso is not None else y
        pred32[name] = run(Xte[:, cols].astype(np.float32))
        pred64[name] = run(Xte[:, cols])
    np.savez_compressed(OUT, models_json=np.array(json.dumps(models)), rows=Xte, names=np.array([s[0] for s in SPECS]),
                        pred32=np.stack([pred32[s[0]] for s in SPECS]), pred64=np.stack([pred64[s[0]] for s in SPECS]))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
