"""Host side of the IRLS fits' window kernel (csrc/k_fit.hip): which instance a frame size takes, and the compiler's SGPR spill code of every new
kernel (tools/check_sgpr_spill_lanes.py, as tests/test_host_cpu.py runs it for the plain <56, 4> kernel).  No GPU."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_NAME = "vistaf-roboskin-vision-integrated-multimodal-sensor_amd"

# kernels.hpp: FitVariant
FITV = ["big", "generic", "generic_div", "col16", "col32", "col48", "col56", "col64", "col48_g4", "col56_g4", "col64_g4",
        "win16", "win32", "win48", "win56", "win32_g4", "win48_g4", "win56_g4"]
# tests/test_kernels_direct.LADDER (that module needs a GPU to import): (h, w) -> the plain instance
LADDER = [((128, 128), "col16"), ((160, 160), "col32"), ((140, 300), "col48"), ((165, 300), "col56"), ((190, 300), "col64"), ((151, 203), "col48_g4"),
          ((224, 224), "col56_g4"), ((256, 256), "col64_g4"), ((320, 320), "generic"), ((512, 512), "big")]
# the window instance is the ladder step below the plain one with the same row-group constant; none below 16 slots, none for the generic and big variants
WINDOW_OF = {"col32": "win16", "col48": "win32", "col56": "win48", "col64": "win56", "col48_g4": "win32_g4", "col56_g4": "win48_g4", "col64_g4": "win56_g4"}


def test_ladder_table_is_the_direct_tests_table():
    text = open(os.path.join(ROOT, "tests", "test_kernels_direct.py")).read()
    got = re.findall(r"\(\((\d+), (\d+)\), \"(\w+)\"\)", text[text.index("LADDER = ["):text.index("FIT_MULT")])
    assert [((int(h), int(w)), v) for h, w, v in got] == LADDER
    assert FITV[:11] == re.search(r"FITV = \[(.*?)\]", text).group(1).replace('"', "").split(", ")


def test_window_instance_table(pkg):
    """vistaf_ftp_test_polyfit_window_instance over the ladder: the window instance where the plain variant has one, else the plain variant itself --
    so polyfit_variant's choice is what it was on every shape (a window instance names its plain variant one to one)"""
    inst = pkg._lib.load().vistaf_ftp_test_polyfit_window_instance
    for (h, w), plain in LADDER:
        for B in (1, 3, 8):
            got = FITV[inst(B, h, w)]
            assert got == WINDOW_OF.get(plain, plain), ((h, w), B, got, plain)
    assert len(set(WINDOW_OF.values())) == len(WINDOW_OF) == 7
    assert inst(0, 224, 224) < 0 and inst(1, 0, 224) < 0


def test_new_kernels_restore_no_undefined_sgpr_spill_lane(tmp_path):
    """every k_robust_polyfit_colwin and k_robust_polyfit_col_retry instance of k_fit.hip, compiled for gfx950: 0 findings"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, PKG_NAME, "csrc")
    asm = str(tmp_path / "k_fit.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", csrc,
                           os.path.join(csrc, "k_fit.hip"), "-o", asm], stderr=subprocess.DEVNULL)
    names = sorted(set(re.findall(r"^(_ZN2vf\d+k_robust_polyfit_col(?:win|_retry)\w+):", open(asm).read(), flags=re.M)))
    assert len(names) == 7 + 8, names                # seven window instances; the chained body at all eight plain sizes
    for name in names:
        out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "check_sgpr_spill_lanes.py"), asm, name], text=True)
        assert out.strip().endswith("0 findings"), out[-2000:]
