"""SURVEY.md §5 'Race detection / sanitizers': the host C of libhsfft.so (planner, plan
registry, pass scheduler, chunking, real and convolution drivers, per-device locks) built
with -fsanitize=address,undefined and with -fsanitize=thread against a null device
(tests/sanitize/null_device.c: computes nothing, touches the first and last element of every
row each launch would read or write), and run through tests/sanitize/sanitize_driver.c:
planner bytes vs the oracle for N <= 3000, every schedule family, edited plans, 8 host
threads sharing plans and cycling the convolution plan cache, and hsfft_exec_multi over 4
null devices (one host thread per device).  CPU only."""
import os
import subprocess

import pytest

import hsfft_testlib as T

SAN = os.path.join(T.REPO, "tests", "sanitize")


@pytest.mark.parametrize("target", ["sanitize_asan", "sanitize_tsan"])
def test_host_code_under_sanitizer(target):
    subprocess.check_call(["make", "-s", "-C", SAN, target])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=1", HSFFT_NULL_NDEV="4")
    r = subprocess.run([os.path.join(SAN, target)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "sanitize: ok" in r.stdout
    assert "runtime error" not in r.stderr        # UBSan
    assert "WARNING: ThreadSanitizer" not in r.stderr


TRACE = os.path.join(T.GOLDEN, "launch_trace.txt")


def record_launch_trace(path):
    """Build tests/sanitize/trace_driver and let the null device write its launch trace to `path`."""
    subprocess.check_call(["make", "-s", "-C", SAN, "trace_driver"])
    if os.path.exists(path):
        os.remove(path)
    env = {k: v for k, v in os.environ.items() if not k.startswith("HSFFT_")}
    env["HSFFT_NULL_TRACE"] = path
    r = subprocess.run([os.path.join(SAN, "trace_driver")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "trace: ok" in r.stdout


def test_launch_trace_matches_recording(tmp_path):
    """The sequence of device-layer calls the host C makes (every pass launch with its geometry,
    signs and hooks, the Bluestein / real / convolution kernels, every copy with its byte count,
    stream selections; which buffers are reused, never an address) for the scenarios of
    tests/sanitize/trace_driver.c is byte for byte what tests/golden/launch_trace.txt recorded.
    Re-record with `python tests/test_sanitize_cpu.py` only when the sequence is meant to change."""
    got = str(tmp_path / "launch_trace.txt")
    record_launch_trace(got)
    assert open(got, "rb").read() == open(TRACE, "rb").read()


if __name__ == "__main__":  # re-record the launch trace fixture
    record_launch_trace(TRACE)
