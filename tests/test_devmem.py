"""The owners of device memory, pinned memory and events (kwok_amd/csrc/devmem.hpp), on the CPU:
tools/devmem_check.cpp (its own main, the header alone over counting stand-ins for the HIP calls)
built with -fsanitize=address,undefined.  It checks the owners' contract case by case (empty, alloc
twice, a failing alloc, grow, moves, swap, release, vectors of structs that hold owners) and runs a
seeded sequence of 10,000 random operations over eight owners in step with a reference model; at exit
nothing is live and no block was freed that was not live."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owners_keep_their_contract_under_sanitizers(tmp_path):
    exe = str(tmp_path / "devmem_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "devmem_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, "10000", "20261"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "10000 operations" in r.stdout and "0 live, 0 bad frees" in r.stdout and "ERROR" not in r.stderr, r.stdout + r.stderr
