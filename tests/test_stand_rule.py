"""The column test of the deep passes' stand rule (csrc/bisbm_stand_rule.hpp) on the CPU.

The sweep kernel's four- and eight-steps passes keep a later step whose inverse-CDF target lies strictly between an earlier
mover's r and s when (D - 1) k fits the target's margin.  The rule is plain C++ in a header the kernel includes;
tests/native/stand_rule_check.cpp includes the same header, moves small columns for real (3..32 blocks, entries 0..6 and a
second tier up to 48, every draw x, D in {4, 8}, 1..D-1 movers applied in order, half of the cases the worst one: all movers on
one side with the largest k the rule lets through) and requires that a step the rule keeps through every pair still has its
target.  It also requires that the run exercised kept and refused candidates and both boundary cases, (D - 1) k == margin and
(D - 1) k == margin + 1, at both depths.  Built with the address and undefined-behaviour sanitizers: a plain program, CPU only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kept_steps_keep_their_targets(tmp_path):
    exe = str(tmp_path / "stand_rule_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                    "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "stand_rule_check.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("D ")]
    assert [l.split(":")[0] for l in lines] == ["D 4", "D 8"], r.stdout
    for l in lines:
        # (the first occurrence of a name is the deep rule's; the two-steps rule's figures follow the bar)
        deep, pair = l.split("|")[0], l.split("|")[1]
        c = {k: int(v) for k, v in re.findall(r"([a-z_]+) (\d+)", deep)}
        assert c["cases"] >= 100000 and c["kept_cases"] > 0, l
        assert c["wrong"] == 0, l
        assert c["kept_pairs"] > 0 and c["refused_pairs"] > 0, l
        assert c["kept_at_boundary"] > 0 and c["refused_at_boundary"] > 0, l
        p = {k: int(v) for k, v in re.findall(r"([a-z_]+) (\d+)", pair)}
        assert p["wrong"] == 0 and p["kept"] > 0 and p["refused"] > 0, l
        assert "packing wrong 0" in l, l
