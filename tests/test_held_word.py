"""The held word of the production sweep kernel (csrc/bisbm_held_word.hpp) on the CPU.

A held handle -- clamped nodes, block constraints, or both -- runs its Metropolis-Hastings sweeps on the production kernel: the
feeder wave forms one 64-bit word per step, bit i set where the node may move to local block i of its type (0 for a clamped
node, the class's row of the bit table cut to the type's window under constraints, all ones otherwise), and the stepping wave
bars a target whose bit is clear.  The window extraction and the barred test are plain C++ in a header the kernel includes;
tests/native/held_word_check.cpp includes the same header and requires, for every (ka, kb) in {1, 2, 31, 32, 33, 63, 64}^2 and
both types, that held_barred(held_word(..), s) is the literal rule -- not cn_allows(bits, class, own0 + s) under a table, always
under a clamp, never without either -- for a class that allows everything, every class that allows one block (bit 0 and bit 63
among them), random classes, each of them clamped too, with noise in the bits of the row outside the window.  Built with the
address and undefined-behaviour sanitizers: a plain program, CPU only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_held_word_is_the_literal_rule(tmp_path):
    exe = str(tmp_path / "held_word_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                    "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "held_word_check.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    c = {k: int(v) for k, v in re.findall(r"([a-z_0-9]+) (\d+)", r.stdout)}
    ks = (1, 2, 31, 32, 33, 63, 64)
    # per (ka, kb, type): 1 + k_own + 8 classes, open and clamped, and the two words without a table; 64 targets per word
    words = sum(2 * (1 + k + 8) + 2 for k in ks) * len(ks) * 2
    assert c["words"] == words and c["targets"] == 64 * words and c["wrong"] == 0, r.stdout
    for name in ("bit0", "bit63", "all_class", "one_block", "clamped_all", "barred", "allowed", "third_word"):
        assert c[name] > 0, r.stdout
