"""The host side of the chirp-z transform (csrc/hsfft_czt.c: hsfft_czt_shape, hsfft_czt_tables and
its rejections, the per-device cache of tables, wrapped chirp and spectrum -- five keys through its
four entries, keys that differ only in df, f0 or the twiddle mode -- and its release by
hsfft_release_scratch and hsfft_finalize) under -fsanitize=address,undefined with leak detection,
against the null device of tests/sanitize: a stand-alone program (tests/sanitize/czt_driver.c)
linked with every host C file of the product, built into a temporary directory.  Nothing is
preloaded and no Python is involved in the program.  CPU only."""
import glob
import os
import subprocess

import hsfft_testlib as T

SAN = os.path.join(T.REPO, "tests", "sanitize")
CSRC = os.path.join(T.PKG_DIR, "csrc")


def test_czt_host_code_under_sanitizer(tmp_path):
    exe = str(tmp_path / "czt_sanitize")
    srcs = sorted(glob.glob(os.path.join(CSRC, "*.c"))) + [os.path.join(SAN, "null_device.c"), os.path.join(SAN, "czt_driver.c")]
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-ffp-contract=off", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(T.REPO, "include"), "-I" + CSRC, "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wno-unused-parameter",
                           "-Werror=implicit-function-declaration", *srcs, "-o", exe, "-lm", "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               HSFFT_NULL_NDEV="4")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "czt sanitize: ok" in r.stdout
    assert "runtime error" not in r.stderr  # UBSan
