"""tools/{knn,kcenter,cluster,moments,resample}_host_check.cpp under the host sanitizers: the argument checks, limits, knobs and
workspace sizing of the embedding ops' C entries, each built as the tool's own header says (hipcc, -Xarch_host
-fsanitize=address,undefined, the listed .hip files and the tool) and run on the CPU as a stand-alone program.  Every call such
a program makes returns before a launch."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
UNITS = {"knn": ("knn",), "kcenter": ("kcenter",), "cluster": ("knn", "cluster"), "moments": ("moments",), "resample": ("resample",)}


@pytest.mark.parametrize("tool", sorted(UNITS))
def test_host_side_under_address_and_ub_sanitizers(tool, tmp_path):
    exe = str(tmp_path / f"{tool}_host_check")
    srcs = [os.path.join("reactranker_amd", "csrc", u + ".hip") for u in UNITS[tool]]
    build = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Xarch_host",
                            "-fsanitize=address,undefined", *srcs, os.path.join("tools", f"{tool}_host_check.cpp"), "-o", exe],
                           cwd=REPO, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], cwd=REPO, capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    assert "host checks clean" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
