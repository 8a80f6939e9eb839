#!/usr/bin/env python3
"""Regenerate tests/golden/strictmath_binades.npz: the per-binade checksums of include/kajo_strictmath.h (and of the IEEE sqrtf) over
every binary32 argument, from the HOST build of the header with the oracle's flags (tools/strictmath_binades.c, gcc -O2 -mfma
-ffp-contract=off). The device sweep (kajo_hip_kat_strictmath_sweep) is compared with these words in tests/test_strictmath.py.

    python tools/make_strictmath_binades.py [--threads 16]

20 tables of 2^32 arguments each: sin, cos, asin, acos, sqrt and pow(x, y) for the fifteen exponents of POW_Y below (the header's own
accuracy list, the Phong exponents e and sampling exponents 1 / (e + 1) of the shipped scenes, an x > 1 case in every table since x
runs over all binary32, and negative y). A quotient such as 1 / 2.2 is the binary32 quotient of the binary32 operands, as the integrator
forms it (kdiv(1.0f, exponent + 1)); the fixture records every y by its bits.

Generation took 272 s on 16 threads: sin and cos 28 s each, asin and acos 19 s, sqrt 5 s, a pow table 8 to 15 s.

Run it again whenever the header changes a result anywhere: the CPU suite recomputes six binades per table and fails with
"regenerate" when the fixture is stale.
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "strictmath_binades.npz")

f32 = np.float32
POW_Y = [("10", f32(10)), ("50", f32(50)), ("100", f32(100)), ("1000", f32(1000)), ("3", f32(3)), ("2.2", f32(2.2)), ("0.5", f32(.5)),
         ("inv2.2", f32(1) / f32(2.2)), ("inv11", f32(1) / f32(11)), ("inv51", f32(1) / f32(51)), ("inv101", f32(1) / f32(101)),
         ("1", f32(1)), ("2", f32(2)), ("neg1", f32(-1)), ("neg2.2", f32(-2.2))]
TABLES = [("sin", 0, f32(0)), ("cos", 1, f32(0)), ("asin", 2, f32(0)), ("acos", 3, f32(0)), ("sqrt", 6, f32(0))] + \
         [("pow_" + name, 4, y) for name, y in POW_Y]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("-o", default=OUT)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="kajo_binades_")
    exe = os.path.join(tmp, "sm_binades")
    subprocess.run(["gcc", "-O2", "-mfma", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tools", "strictmath_binades.c"), "-lm", "-lpthread"], check=True)
    sums, t0 = [], time.time()
    for name, fn, y in TABLES:
        t1 = time.time()
        ybits = "%08x" % int(np.array(y, f32).view(np.uint32))
        out = subprocess.run([exe, str(fn), ybits, str(a.threads)], check=True, capture_output=True, text=True).stdout.split()
        assert len(out) == 1024, len(out)
        sums.append(np.array([int(w, 16) for w in out], np.uint64).reshape(512, 2))  # row = binade, columns A, B
        print("%-10s y = %-12r %5.1f s" % (name, float(y), time.time() - t1), flush=True)
    # names[t], fn[t], ybits[t] (y's binary32 bits), sums[t, binade, 0 / 1]: binade = sign * 256 + biased exponent; A = sum bits(r),
    # B = sum bits(r) * (2 mantissa + 1), mod 2^64, a NaN as 0x7fc00000
    np.savez_compressed(a.o, names=np.array([t[0] for t in TABLES]), fn=np.array([t[1] for t in TABLES], np.int32),
                        ybits=np.array([t[2] for t in TABLES], f32).view(np.uint32), sums=np.array(sums))
    print("wrote %s (%d bytes) in %.0f s on %d threads" % (a.o, os.path.getsize(a.o), time.time() - t0, a.threads))
    return 0


if __name__ == "__main__":
    sys.exit(main())
