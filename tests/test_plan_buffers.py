"""The owning arena of the solver plans' device and pinned blocks (csrc/plan_buffers.hpp, device-free) under AddressSanitizer and
UndefinedBehaviorSanitizer on the CPU, leak detection on: a create-shaped script over counting fakes of the device layer, with
every one of its allocations failing in turn (tests/plan_buffers.cpp)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "plan_buffers.cpp")


def test_plan_buffers_under_sanitizer(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "plan_buffers")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert "plan buffers OK" in log and "ERROR: AddressSanitizer" not in log and "runtime error" not in log, log[-4000:]
