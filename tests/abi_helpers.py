"""What the tests of the read-outs outside include/*.h share (test_outlines, test_textures, test_matches, test_centrelines, test_lobes): a
header's prototypes held against a signature table of _lib -- the rule of tests/test_abi_surface.py, whose prototype count those headers stay
out of -- and the two bit-equality rules."""
import ctypes
import re

import numpy as np


def _prototypes(text):
    """name -> (return type text, [parameter text]) of every vistaf_* function `text` declares, comments and preprocessor lines stripped"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = "\n".join(ln for ln in re.sub(r"//[^\n]*", " ", text).split("\n") if not ln.lstrip().startswith("#"))
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(vistaf_\w+)\s*\(([^()]*)\)\s*;", text):
        assert name not in protos
        protos[name] = (" ".join(ret.split()), [" ".join(p.split()) for p in params.split(",")])
    return protos


def _hold_against(protos, table, lib):
    """the prototypes and the table name the same functions, every parameter and return type has the ctypes type of its kind (pointer <->
    pointer, scalar <-> the scalar of the same kind), and the loaded library carries the table's argtypes"""
    scalars = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "double": ctypes.c_double, "float": ctypes.c_float, "int64_t": ctypes.c_int64,
               "size_t": ctypes.c_size_t}

    def matches(c_text, ctype):
        if "*" in c_text:
            return ctype in (ctypes.c_void_p, ctypes.c_char_p) or isinstance(ctype, type(ctypes.POINTER(ctypes.c_int)))
        words = [w for w in re.findall(r"\w+", c_text) if w not in ("const", "unsigned", "signed")]
        kind = next((w for w in words if w in scalars), None)
        assert kind is not None, c_text
        return ctype is scalars[kind]
    assert sorted(protos) == sorted(table)
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert len(argtypes) == len(params), name
        for i, (p, a) in enumerate(zip(params, argtypes)):
            assert matches(p, a), (name, i, p, a)
        assert restype is not None and matches(ret, restype)
        assert hasattr(lib, name) and getattr(lib, name).argtypes == argtypes


def _same_bits(a, b):
    """the same shape and every byte equal, the bits of a NaN included (test_outlines, test_matches)"""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _same_f64_bits(a, b):
    """as float64: NaN in the same places, bit for bit elsewhere (test_centrelines, test_lobes: against a NumPy reference, whose NaN may
    carry other bits)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb])
