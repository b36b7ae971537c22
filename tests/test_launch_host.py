"""No GPU needed: the per-device one-time state of csrc/launch.h (device_cus, DeviceOnce) under 8 racing threads.

tests/native/launch_host.hip is a stand-alone program (its own main) that includes launch.h; it is built twice, plain and with
ThreadSanitizer on the host code, and both binaries must exit 0.  The sanitizer build runs with the GPUs hidden, so that it checks
launch.h's own code on the fallback path (device 0, 256 compute units) on every machine and never opens a device; the plain build runs
in the machine's own environment and checks the fallbacks where there is no GPU, the queried values where there is one."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "launch_host.hip")


def _build(out, extra=()):
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", *extra, SRC, "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def _run(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.stdout, r.stderr)
    return r.stdout


@pytest.fixture(scope="module")
def hipcc():
    assert shutil.which("hipcc"), "hipcc not found on PATH"


def test_device_state_is_consistent_across_threads(hipcc, tmp_path):
    out = _run(_build(str(tmp_path / "launch_host")))
    assert "ok" in out
    if "no GPU" in out:
        assert "device 0, 256 compute units" in out


def test_device_state_is_race_free_under_thread_sanitizer(hipcc, tmp_path):
    exe = _build(str(tmp_path / "launch_host_tsan"), ["-Xarch_host", "-fsanitize=thread"])
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    out = _run(exe, env)
    assert "no GPU, device 0, 256 compute units" in out and "ok" in out
