"""tools/moments_host_check.cpp under the host sanitizers: the argument checks, limits, chunk function and workspace sizing of
csrc/moments.hip, built as the tool's header says (hipcc, -Xarch_host -fsanitize=address,undefined) and run on the CPU as a
stand-alone program.  Every call it makes returns before a launch."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_moments_host_side_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "moments_host_check")
    build = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Xarch_host",
                            "-fsanitize=address,undefined", os.path.join("reactranker_amd", "csrc", "moments.hip"),
                            os.path.join("tools", "moments_host_check.cpp"), "-o", exe],
                           cwd=REPO, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], cwd=REPO, capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    assert "host checks clean" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
