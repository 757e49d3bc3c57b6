"""csrc/p3d_plane_stage.h on the CPU: tests/host_checks/plane_stage_check.cpp, a stand-alone program with stub buffers in
place of the scene handle's, built with the address and undefined-behaviour sanitizers and run directly.  It checks the
declare -> prepare -> run order, that a refused call allocates nothing, and the fixed-capacity overflow check."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "u_4a_2s_p3d_raytracer_template2_amd", "csrc")


def test_plane_stage_under_sanitizers(tmp_path):
    exe = str(tmp_path / "plane_stage_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(REPO, "include"), "-I" + CSRC, os.path.join(REPO, "tests", "host_checks", "plane_stage_check.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "plane_stage_check ok" in out.stdout, out.stdout + out.stderr
