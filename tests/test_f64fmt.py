"""The shared host / device float formatter (kwok_amd/csrc/f64fmt.hpp) through its host export
kwk_expo_format_f64, and the fixed go_float, against Go's strconv.AppendFloat(v, 'g', -1, 64) rule
restated here from repr's own shortest digits and exponent (CPython's repr and Go's shortest
formatting both give the shortest round-trip digits, closest to the value)."""
import math
import struct

import numpy as np
import pytest

from kwok_amd.host.metrics import go_float

EDGES = [0.0, -0.0, float("nan"), float("inf"), float("-inf"),
         5e-324, 2.2250738585072014e-308, 1.7976931348623157e308,
         1e-5, 0.0001, 99999.99999999999, 999999.0, 999999.9999999999, 1e6, 1234567.0,
         1e21, 1e22, 1e23, float(2**53 + 2), 0.1 + 0.2, 9.5, 134217728.0, 1.5e-7]
# 1e23 and neighbours: the exact value's decimal exponent is one below the shortest digits'
EXPONENT_NEIGHBOURS = [1e23, -1e23, 9.999999999999999e22, 1.0000000000000001e23, 2e23, 1e-23, 5e-324, 1e22, 1e24,
                       8.41e21, 2.0**63, 2.0**64, 9.5e-5, 1e-4, 9.999999999999999e-5]


def go_g(v: float) -> str:
    """strconv.FormatFloat(v, 'g', -1, 64): %e when the exponent X of the shortest digits is < -4
    or >= 6 (ftoa.go: eprec = 6 for 'shortest'), the exponent with a sign and two digits at least."""
    if math.isnan(v):
        return "NaN"
    if math.isinf(v):
        return "+Inf" if v > 0 else "-Inf"
    if v == 0:
        return "-0" if math.copysign(1.0, v) < 0 else "0"
    mant, _, e = repr(abs(v)).partition("e")
    ip, _, fp = mant.partition(".")
    all_digits = ip + fp
    lead = len(all_digits) - len(all_digits.lstrip("0"))
    d = all_digits.strip("0")
    x = int(e or 0) + len(ip) - 1 - lead
    if x < -4 or x >= 6:
        out = d[0] + ("." + d[1:] if len(d) > 1 else "") + "e" + ("-" if x < 0 else "+") + "%02d" % abs(x)
    elif x >= 0:
        out = d[:x + 1].ljust(x + 1, "0") + ("." + d[x + 1:] if len(d) > x + 1 else "")
    else:
        out = "0." + "0" * (-x - 1) + d
    return ("-" if v < 0 else "") + out


def random_values():
    rng = np.random.default_rng(20240607)
    bits = rng.integers(0, 2**64, size=200_000, dtype=np.uint64)
    vals = list(bits.view(np.float64))
    # short decimals of the kind usage sums produce: milli-cores, MiB multiples, seconds
    mag = rng.integers(0, 10, size=50_000)
    dec = rng.integers(0, 7, size=50_000)
    frac = rng.random(50_000)
    vals += [round(float(f) * 10.0 ** int(m), int(d)) for f, m, d in zip(frac, mag, dec)]
    vals += [float(k) * 0.001 for k in range(0, 4000, 7)] + [float(k) * 1048576.0 for k in range(0, 3000, 11)]
    return vals


def test_restated_rule_on_known_go_outputs():
    known = {1e23: "1e+23", 1e21: "1e+21", 1e22: "1e+22", 1e6: "1e+06", 999999.0: "999999", 1234567.0: "1.234567e+06",
             0.0001: "0.0001", 1e-5: "1e-05", 5e-324: "5e-324", 1.7976931348623157e308: "1.7976931348623157e+308",
             0.1 + 0.2: "0.30000000000000004", float(2**53 + 2): "9.007199254740994e+15", 9.5: "9.5",
             134217728.0: "1.34217728e+08", 1.5e-7: "1.5e-07", 99999.99999999999: "99999.99999999999"}
    for v, want in known.items():
        assert go_g(v) == want, v


def test_committed_tables_are_the_generators():
    """f64fmt_tables.hpp is what tools/gen_f64fmt_tables.py computes (big-int arithmetic)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, os.path.join(root, "tools", "gen_f64fmt_tables.py"), "--check"]).returncode == 0


@pytest.fixture(scope="module")
def fmt():
    from kwok_amd import build
    build.build()
    from kwok_amd.host import expo
    return expo.format_f64


def test_native_formatter_edges(fmt):
    for v in EDGES + EXPONENT_NEIGHBOURS + [-x for x in EDGES if x == x]:
        assert fmt(v) == go_g(v).encode(), v
    assert fmt(-1.7976931348623157e308) == b"-1.7976931348623157e+308"  # the longest: 24 bytes
    assert fmt(1e23) == b"1e+23"


def test_native_formatter_random(fmt):
    import ctypes as C
    from kwok_amd.host import expo
    L = expo.lib()
    buf = C.create_string_buffer(32)
    bad = []
    for v in random_values():
        v = float(v)
        n = L.kwk_expo_format_f64(v, buf)
        assert n <= 24
        got = buf.raw[:n]
        if got != go_g(v).encode():
            bad.append((struct.pack("<d", v).hex(), got, go_g(v)))
    assert not bad, bad[:10]


def test_go_float_fixed_agrees():
    assert go_float(1e23) == "1e+23"  # was 1e+22: the exponent came from the exact value, not the shortest digits
    for v in EDGES + EXPONENT_NEIGHBOURS:
        assert go_float(v) == go_g(v), v
    bad = [v for v in random_values() if go_float(float(v)) != go_g(float(v))]
    assert not bad, bad[:10]
