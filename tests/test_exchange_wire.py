"""csrc/gs_exchange_wire.h, the one statement of the per-hop exchange's layouts
(size row, count readback, device counter blocks, broadcast chunk, block sizes,
send and receive plans, dials): tests/exchange_wire_check.cpp checks it against
the literal index arithmetic both ends of the exchange used to write out, and
checks that what a receive plan expects from a rank is what that rank's send
plan sends, at world 1, 2, 3 and 8.  Host C++ only: built with g++ under
AddressSanitizer and UBSan and run directly (CPU, a second or two)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wire_layouts_and_plans(tmp_path):
    exe = tmp_path / "exchange_wire_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "go-libp2p-pubsub_amd", "csrc"),
                    os.path.join(REPO, "tests", "exchange_wire_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=180)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    word, checks = out.stdout.split()
    assert word == "ok" and int(checks) > 10000
