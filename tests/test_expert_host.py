"""CPU: tests/host/expert_host_check.cpp -- every refusal of csrc/expert.hip -- built as a program of its own with the host side
under AddressSanitizer and UBSan (the device side is compiled as always and never runs: every refusal returns before a launch), and
run.  Needs no GPU; nothing here is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "autonomous_driving_with_diffusion_model_amd", "csrc")


def test_the_refusals_of_the_expert_hold_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "expert_host_check")
    build = subprocess.run(["hipcc", "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function",
                            "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                            "-x", "hip", os.path.join(CSRC, "expert.hip"), os.path.join(ROOT, "tests", "host", "expert_host_check.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    with open(exe, "rb") as f:
        image = f.read()
    assert b"__asan_init" in image and b"__ubsan_handle" in image            # the host side really is instrumented
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert "every refusal held" in run.stdout
