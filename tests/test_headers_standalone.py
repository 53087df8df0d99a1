"""Every device header under csrc/ compiles as the only include of a translation unit.

The device code is layered (rtg_math < rtg_isect < rtg_walk < rtg_anyhit /
rtg_shade < rtg_frame < rtg_shadow_kernels, rtg_common.hpp the umbrella over them): a header
includes what it uses and nothing above it.  A header that leans on its includer's earlier includes
compiles inside the library and fails here.  Device side only, gfx950, syntax only, with the
Makefile's -std and include paths; no GPU needed."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "advanced-cpu-raytracing_amd")
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(PKG, "csrc", "rtg_*.hpp")))


def hipcc():
    cand = os.environ.get("HIPCC") or shutil.which("hipcc") or os.path.join(
        os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    return cand if os.path.exists(cand) else None


def makefile_std():
    flags = re.search(r"^HIPFLAGS\s*:=(.*(?:\\\n.*)*)", open(os.path.join(PKG, "Makefile")).read(), re.M).group(1)
    return re.search(r"-std=\S+", flags).group(0)


def test_the_layered_headers_are_there():
    for h in ("rtg_common.hpp", "rtg_math.hpp", "rtg_isect.hpp", "rtg_walk.hpp", "rtg_anyhit.hpp", "rtg_shade.hpp",
              "rtg_frame.hpp", "rtg_shadow_kernels.hpp"):
        assert h in HEADERS, h


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header, tmp_path):
    cc = hipcc()
    if not cc:
        pytest.skip("no hipcc")
    tu = tmp_path / "tu.hip"
    tu.write_text('#include "%s"\n' % header)
    r = subprocess.run([cc, "-x", "hip", "--offload-arch=gfx950", "--cuda-device-only", "-fsyntax-only", makefile_std(),
                        "-Wall", "-Wno-unused-parameter", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(PKG, "csrc"), str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
