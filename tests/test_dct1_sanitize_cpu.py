"""The host side of the type-I cosine and sine transforms (csrc/hsfft_dct1.c: the kind and length rule
at both ends of both kinds, hsfft_dct1_shape, every rejection of hsfft_dct1_batched and
hsfft_dct1_2d_batched -- pointers, batch, totals at the 2^40 bound, overlap at the edges of the ranges
and at the top of the address space -- and the chunk rule at several knob values) under
-fsanitize=address,undefined with leak detection, against the null device of tests/sanitize: a
stand-alone program (tests/sanitize/dct1_driver.c) linked with every host C file of the product,
built into a temporary directory.  Nothing is preloaded and no Python is involved in the program.
CPU only."""
import glob
import os
import subprocess

import hsfft_testlib as T

SAN = os.path.join(T.REPO, "tests", "sanitize")
CSRC = os.path.join(T.PKG_DIR, "csrc")


def test_dct1_host_code_under_sanitizer(tmp_path):
    exe = str(tmp_path / "dct1_sanitize")
    srcs = sorted(glob.glob(os.path.join(CSRC, "*.c"))) + [os.path.join(SAN, "null_device.c"), os.path.join(SAN, "dct1_driver.c")]
    assert os.path.join(CSRC, "hsfft_dct1.c") in srcs
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-ffp-contract=off", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(T.REPO, "include"), "-I" + CSRC, "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wno-unused-parameter",
                           "-Werror=implicit-function-declaration", *srcs, "-o", exe, "-lm", "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               HSFFT_NULL_NDEV="4")
    env.pop("HSFFT_DCT_CHUNK_MB", None)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "dct1 sanitize: ok" in r.stdout
    assert "runtime error" not in r.stderr  # UBSan
