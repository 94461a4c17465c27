"""The temperature regressors (last slice of the temperature modality) from exported parameters.

Reference interface mirrored: Code/temperature_sensor.py
  * `TempModel.predict(X)`                  (:230-243): StandardScaler -> PolynomialFeatures -> HuberRegressor, optionally followed by an
                                            IsotonicRegression calibrator (assumed to compose as iso(pipeline(X)), include/vistaf_tempmodel.h)
  * `predict_map_for_mask(planes, mask)`    (:295): the model on the feature planes under a mask, NaN elsewhere
backed by `vistaf_tmodel_*` of libvistaf_ftp.so (include/vistaf_tempmodel.h), which also states the arithmetic contract.

The library never imports scikit-learn or joblib and never unpickles.  The caller loads its fitted objects in its own environment and
hands them to `TempModel.from_sklearn`, which reads attributes only, or stores them once with `to_json` and reloads them with `from_json`.
"""
from __future__ import annotations

import ctypes
import itertools
import json
import math
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._handle import Handle, call, stream

FEATURE_NAMES = ("L", "a", "b", "gray")            # plane order of the C ABI (VISTAF_TMODEL_PLANE_*)
DEFAULT_FEATURES = {3: ("L", "a", "b"), 4: ("L", "a", "b", "gray")}   # the colour and the black model of the reference
MAX_FEATURES, MAX_DEGREE, MAX_TERMS = 4, 4, 70
SCHEMA_KEY, SCHEMA_VERSION = "vistaf_tempmodel", 1
OUT_OF_BOUNDS = {"clip": 0, "nan": 1}


def polynomial_powers(n_features: int, degree: int, include_bias: bool = True) -> np.ndarray:
    """PolynomialFeatures(degree, include_bias=...).fit(X with n_features columns).powers_ -- the term order of every model here"""
    rows = []
    for d in range(0 if include_bias else 1, int(degree) + 1):
        for comb in itertools.combinations_with_replacement(range(int(n_features)), d):
            rows.append(np.bincount(np.asarray(comb, dtype=np.int64), minlength=int(n_features)))
    return np.asarray(rows, dtype=np.int32).reshape(-1, int(n_features))


def _f64_vector(v, n: int, what: str) -> np.ndarray:
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.shape != (n,):
        raise ValueError(f"{what} must hold {n} values, got {a.shape[0]}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{what} must be finite")
    return a


class _DeviceModel(Handle):
    """The copy of a model's parameters on one device (vistaf_tmodel_create)"""
    _destroy = "vistaf_tmodel_destroy"

    def __init__(self, device: torch.device, *params):
        self._open(device, need_device=False)
        self._call("vistaf_tmodel_create", *params, ctypes.byref(self._h))


class TempModel:
    """One fitted temperature regressor as plain arrays (see include/vistaf_tempmodel.h for the arithmetic).

    features   ordered subset of ("L", "a", "b", "gray")
    mean, scale, with_mean, with_std           StandardScaler.mean_, .scale_ and flags
    powers [T, F]                               PolynomialFeatures.powers_ (bias row included when include_bias)
    coef [T], intercept                         the final linear step's coef_ / intercept_
    isotonic   None or dict(x_thresholds, y_thresholds, x_min, x_max, out_of_bounds in {"clip", "nan"})
    The device copy of the parameters is made once per device, on first use.
    """

    def __init__(self, features: Sequence[str], mean, scale, with_mean: bool, with_std: bool, powers, coef, intercept: float,
                 isotonic: Optional[Dict[str, Any]] = None):
        feats = tuple(str(f) for f in features)
        if not 1 <= len(feats) <= MAX_FEATURES:
            raise ValueError(f"a model takes 1..{MAX_FEATURES} features, got {len(feats)}")
        if any(f not in FEATURE_NAMES for f in feats) or len(set(feats)) != len(feats):
            raise ValueError(f"features must be distinct names out of {FEATURE_NAMES}, got {feats}")
        F = len(feats)
        self.features = feats
        self.with_mean, self.with_std = bool(with_mean), bool(with_std)
        self.mean = _f64_vector(np.zeros(F) if mean is None else mean, F, "mean")
        self.scale = _f64_vector(np.ones(F) if scale is None else scale, F, "scale")
        if self.with_std and not np.all(self.scale > 0):
            raise ValueError("scale must be > 0")
        pw = np.asarray(powers)
        if pw.ndim != 2 or pw.shape[1] != F:
            raise ValueError(f"powers must be [T, {F}], got shape {pw.shape}")
        if not np.issubdtype(pw.dtype, np.integer):
            if not np.all(pw == np.round(pw)):
                raise ValueError("powers must be integers")
        pw = pw.astype(np.int32)
        if pw.shape[0] < 1 or pw.shape[0] > MAX_TERMS:
            raise ValueError(f"a model has 1..{MAX_TERMS} terms, got {pw.shape[0]}")
        if np.any(pw < 0) or np.any(pw.sum(axis=1) > MAX_DEGREE):
            raise ValueError(f"term degree must be 0..{MAX_DEGREE}")
        if len({tuple(r) for r in pw.tolist()}) != pw.shape[0]:
            raise ValueError("powers has a repeated row")
        self.powers = pw
        self.coef = _f64_vector(coef, pw.shape[0], "coef")
        self.intercept = float(intercept)
        if not math.isfinite(self.intercept):
            raise ValueError("intercept must be finite")
        self.isotonic = None
        if isotonic is not None:
            xt = np.asarray(isotonic["x_thresholds"], dtype=np.float64).reshape(-1)
            K = xt.shape[0]
            if K < 1:
                raise ValueError("isotonic table is empty")
            xt = _f64_vector(xt, K, "isotonic x_thresholds")
            yt = _f64_vector(isotonic["y_thresholds"], K, "isotonic y_thresholds")
            if K > 1 and not np.all(np.diff(xt) > 0):
                raise ValueError("isotonic x_thresholds must be strictly increasing")
            xmin, xmax = float(isotonic["x_min"]), float(isotonic["x_max"])
            if not (math.isfinite(xmin) and math.isfinite(xmax)) or xmin > xmax:
                raise ValueError("isotonic x_min / x_max must be finite with x_min <= x_max")
            oob = str(isotonic["out_of_bounds"])
            if oob not in OUT_OF_BOUNDS:
                raise ValueError(f"isotonic out_of_bounds must be 'clip' or 'nan', got {oob!r}")
            self.isotonic = {"x_thresholds": xt, "y_thresholds": yt, "x_min": xmin, "x_max": xmax, "out_of_bounds": oob}
        self._handles: Dict[int, _DeviceModel] = {}

    @property
    def degree(self) -> int:
        return int(self.powers.sum(axis=1).max())

    # ---- constructors -------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_sklearn(cls, pipeline, isotonic=None, features: Optional[Sequence[str]] = None) -> "TempModel":
        """From a fitted Pipeline(StandardScaler, PolynomialFeatures, linear regressor) and an optional fitted IsotonicRegression.
        Reads attributes only (mean_, scale_, powers_, coef_, intercept_, X_thresholds_, y_thresholds_, X_min_, X_max_, out_of_bounds);
        anything outside the family the reference trains raises ValueError."""
        steps = getattr(pipeline, "steps", None)
        if steps is None:
            raise ValueError("expected a fitted scikit-learn Pipeline")
        if len(steps) != 3:
            raise ValueError(f"expected exactly StandardScaler -> PolynomialFeatures -> regressor, got {len(steps)} steps")
        sc, pf, reg = (s[1] for s in steps)
        if not all(hasattr(sc, a) for a in ("with_mean", "with_std", "mean_", "scale_")):
            raise ValueError("first step is not a fitted StandardScaler")
        if not hasattr(pf, "powers_"):
            raise ValueError("second step is not a fitted PolynomialFeatures")
        if getattr(pf, "interaction_only", False):
            raise ValueError("PolynomialFeatures(interaction_only=True) is not supported")
        if not (hasattr(reg, "coef_") and hasattr(reg, "intercept_")):
            raise ValueError("final step has no coef_ / intercept_")
        powers = np.asarray(pf.powers_)
        F = powers.shape[1]
        if F > MAX_FEATURES:
            raise ValueError(f"more than {MAX_FEATURES} features ({F})")
        if int(powers.sum(axis=1).max()) > MAX_DEGREE:
            raise ValueError(f"degree above {MAX_DEGREE}")
        if powers.shape[0] > MAX_TERMS:
            raise ValueError(f"more than {MAX_TERMS} terms ({powers.shape[0]})")
        coef = np.asarray(reg.coef_)
        if coef.dtype != np.float64 or coef.ndim != 1:
            raise ValueError("coef_ must be a float64 vector (a single-output model fitted in float64)")
        icpt = np.asarray(reg.intercept_, dtype=np.float64).reshape(-1)
        if icpt.shape != (1,):
            raise ValueError("intercept_ must be a scalar")
        if features is None:
            if F not in DEFAULT_FEATURES:
                raise ValueError(f"pass features= for a {F}-feature model")
            features = DEFAULT_FEATURES[F]
        iso = None
        if isotonic is not None:
            for a in ("X_thresholds_", "y_thresholds_", "X_min_", "X_max_", "out_of_bounds"):
                if not hasattr(isotonic, a):
                    raise ValueError(f"isotonic calibrator is not a fitted IsotonicRegression (no {a})")
            if isotonic.out_of_bounds == "raise":
                raise ValueError("IsotonicRegression(out_of_bounds='raise') is not supported")
            xt, yt = np.asarray(isotonic.X_thresholds_), np.asarray(isotonic.y_thresholds_)
            if xt.dtype != np.float64 or yt.dtype != np.float64:
                raise ValueError("isotonic thresholds must be float64 (a calibrator fitted on the float64 predictions)")
            iso = {"x_thresholds": xt, "y_thresholds": yt, "x_min": float(isotonic.X_min_), "x_max": float(isotonic.X_max_),
                   "out_of_bounds": isotonic.out_of_bounds}
        return cls(features, sc.mean_, sc.scale_, sc.with_mean, sc.with_std, powers, coef, float(icpt[0]), iso)

    def to_dict(self) -> Dict[str, Any]:
        d = {SCHEMA_KEY: SCHEMA_VERSION, "features": list(self.features),
             "scaler": {"mean": [float(v) for v in self.mean], "scale": [float(v) for v in self.scale],
                        "with_mean": self.with_mean, "with_std": self.with_std},
             "powers": self.powers.tolist(), "coef": [float(v) for v in self.coef], "intercept": self.intercept, "isotonic": None}
        if self.isotonic is not None:
            i = self.isotonic
            d["isotonic"] = {"x_thresholds": [float(v) for v in i["x_thresholds"]], "y_thresholds": [float(v) for v in i["y_thresholds"]],
                             "x_min": i["x_min"], "x_max": i["x_max"], "out_of_bounds": i["out_of_bounds"]}
        return d

    def to_json(self, path: Optional[str] = None) -> str:
        """JSON text (floats as the shortest repr that reads back to the same double); written to `path` when given"""
        text = json.dumps(self.to_dict(), indent=1, allow_nan=False)
        if path is not None:
            with open(path, "w") as f:
                f.write(text)
        return text

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "TempModel":
        if d.get(SCHEMA_KEY) != SCHEMA_VERSION:
            raise ValueError(f"not a {SCHEMA_KEY} version {SCHEMA_VERSION} document")
        s = d["scaler"]
        return cls(d["features"], s["mean"], s["scale"], s["with_mean"], s["with_std"], np.asarray(d["powers"], dtype=np.int64), d["coef"],
                   d["intercept"], d.get("isotonic"))

    @classmethod
    def from_json(cls, src: str) -> "TempModel":
        """From JSON text or the path of a file written by to_json"""
        text = src if src.lstrip().startswith("{") else open(src).read()
        return cls.from_dict(json.loads(text))

    # ---- device ---------------------------------------------------------------------------------------------------------------------
    def _handle(self, device: torch.device) -> ctypes.c_void_p:
        idx = device.index if device.index is not None else torch.cuda.current_device()
        h = self._handles.get(idx)
        if h is None:
            i32p, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
            planes = np.asarray([FEATURE_NAMES.index(f) for f in self.features], dtype=np.int32)
            powers = np.ascontiguousarray(self.powers, dtype=np.int32)
            iso = self.isotonic
            xt = np.ascontiguousarray(iso["x_thresholds"]) if iso else None
            yt = np.ascontiguousarray(iso["y_thresholds"]) if iso else None
            h = self._handles[idx] = _DeviceModel(
                torch.device("cuda", idx), len(self.features), planes.ctypes.data_as(i32p), self.mean.ctypes.data_as(dp),
                self.scale.ctypes.data_as(dp), int(self.with_mean), int(self.with_std), powers.shape[0], powers.ctypes.data_as(i32p),
                self.coef.ctypes.data_as(dp), self.intercept, xt.shape[0] if iso else 0, xt.ctypes.data_as(dp) if iso else None,
                yt.ctypes.data_as(dp) if iso else None, iso["x_min"] if iso else 0.0, iso["x_max"] if iso else 0.0,
                OUT_OF_BOUNDS[iso["out_of_bounds"]] if iso else 0)
        return h._h

    def close(self):
        handles, self._handles = getattr(self, "_handles", {}), {}
        for h in handles.values():
            h.close()

    # ---- prediction -----------------------------------------------------------------------------------------------------------------
    def predict(self, X, device=None):
        """Drop-in for TempModel.predict(X) (:230-243): X [N, F] rows (NumPy or a device tensor), float32 rows in float32 arithmetic
        and float64 rows in float64, as scikit-learn does; other dtypes are converted to float64.  Returns float64 [N], a NumPy array
        for host rows and a device tensor for device rows."""
        on_dev = torch.is_tensor(X) and X.is_cuda
        dev = X.device if on_dev else torch.device(device or "cuda:0")
        x = X if torch.is_tensor(X) else torch.from_numpy(np.asarray(X))
        if x.dtype not in (torch.float32, torch.float64):
            x = x.to(torch.float64)
        if x.dim() != 2 or x.shape[1] != len(self.features):
            raise ValueError(f"X must be [N, {len(self.features)}], got {tuple(x.shape)}")
        x = x.to(dev).contiguous()
        out = torch.empty(x.shape[0], dtype=torch.float64, device=dev)
        h = self._handle(dev)
        call(dev, "vistaf_tmodel_predict_rows", h, x.data_ptr(), 0 if x.dtype == torch.float32 else 1, x.shape[0], out.data_ptr(), stream(dev))
        return out if on_dev else out.cpu().numpy()

    def predict_map_for_mask(self, planes, mask, device=None):
        """Drop-in for predict_map_for_mask(planes, mask) (:295): float32 [H, W], the model where mask is set, NaN elsewhere"""
        return predict_maps(planes, (self, mask), device=device)[0]


def predict_map_for_mask(model: TempModel, planes, mask, device=None):
    """predict_map_for_mask (:295) with the model passed explicitly"""
    return model.predict_map_for_mask(planes, mask, device=device)


def predict_maps(planes, *pairs: Tuple[TempModel, Any], device=None):
    """One pass over the planes for one or two (model, mask) pairs, e.g. (wide model, its mask), (colour model, colour support):
    returns a tuple of float32 [H, W] maps, NaN outside each mask -- the wide and the colour map fuse_maps_per_pixel takes.
    `planes` holds float32 [H, W] "L" / "a" / "b" / "gray" as NumPy arrays (maps come back as NumPy) or as device tensors such as
    TempSegmenter.feature_planes_device returns (maps stay on the device, no host round trip)."""
    if not 1 <= len(pairs) <= 2:
        raise ValueError("predict_maps takes one or two (model, mask) pairs")
    names = sorted({f for m, _ in pairs for f in m.features}, key=FEATURE_NAMES.index)
    missing = [n for n in names if n not in planes]
    if missing:
        raise ValueError(f"planes lacks {missing}")
    used = [planes[n] for n in names]
    on_dev = any(torch.is_tensor(p) and p.is_cuda for p in used)
    if device is None:
        device = next((p.device for p in used if torch.is_tensor(p) and p.is_cuda), None) or "cuda:0"
    dev = torch.device(device)
    shape = tuple(int(v) for v in used[0].shape)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"planes must be [H, W] with H, W >= 1, got {shape}")
    dplanes = {}
    for n in names:
        t = planes[n] if torch.is_tensor(planes[n]) else torch.from_numpy(np.asarray(planes[n]))
        if t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise ValueError(f"plane {n!r} must be float32 {list(shape)}")
        dplanes[n] = t.to(dev).contiguous()
    masks, outs, handles = [], [], []
    for model, mask in pairs:
        m = mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask)))
        if tuple(m.shape) != shape:
            raise ValueError("mask shape does not match the planes")
        masks.append((m.to(dev) != 0).to(torch.uint8).contiguous())
        outs.append(torch.empty(shape, dtype=torch.float32, device=dev))
        handles.append(model._handle(dev))
    n = len(pairs)
    VP = ctypes.c_void_p
    c_models = (VP * n)(*[h.value for h in handles])
    c_masks = (VP * n)(*[m.data_ptr() for m in masks])
    c_outs = (VP * n)(*[o.data_ptr() for o in outs])
    c_planes = (VP * 4)(*[dplanes[k].data_ptr() if k in dplanes else None for k in FEATURE_NAMES])
    call(dev, "vistaf_tmodel_predict_maps", n, c_models, c_masks, c_outs, c_planes, shape[0], shape[1], stream(dev))
    return tuple(outs) if on_dev else tuple(o.cpu().numpy() for o in outs)
