"""The composite id table of the fused 1-byte sweep (kwok_amd/csrc/id8_compose.hpp), on the CPU:
tools/id8_compose_check.cpp (its own main, the header alone) built with -fsanitize=address,undefined
compares every row for 2 and 4 steps against the one-step rule iterated, restated in the checker, for
seeded random id tables and the hand-made cases (an id that fires the same stage at every step, ids
that leave the list at each possible step, a table without a need bit)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_composite_rows_equal_the_iterated_one_step_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "id8_compose_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "id8_compose_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, "3000", "20261"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "3003 tables, 0 bad" in r.stdout and "ERROR" not in r.stderr, r.stdout + r.stderr
