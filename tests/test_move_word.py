"""step_quad32's one-stage update of the register copies of m_r / n_r (csrc/bisbm_move_word.hpp) on the CPU.

After the verdicts the four-steps pass of 17..32 blocks no longer walks its movers one by one: every row of lanes has formed
its step's contribution to the lane's two blocks beforehand (move_word), the movers' words are combined across the rows with
two lane swaps (combine_move_words) and split into the two addends.  tests/native/move_word_check.cpp includes the header the
kernel includes, models the wave as an array and the swaps as the instructions' definitions, and compares with the per-mover
loop for every subset of movers with pairwise disjoint block sets, with 32, 27, 20 and 17 blocks and degrees 1, 127, 128 and
255 -- the m_r addend is no signed byte.  Built with the address and undefined-behaviour sanitizers: a plain program, CPU only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_combined_update_equals_the_per_mover_loop(tmp_path):
    exe = str(tmp_path / "move_word_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                    "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "move_word_check.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert [l.split(":")[0] for l in lines] == ["quad32", "quad27", "quad20", "quad17"], r.stdout
    for l in lines:
        c = {k: int(v) for k, v in re.findall(r"([a-z_]+) (\d+)", l.split(" movers")[0])}
        assert c["cases"] >= 50000 and c["wrong"] == 0 and c["big_degree_movers"] > 0, l
        movers = [int(v) for v in l.split(" movers")[1].split()]
        assert len(movers) == 5 and all(v > 0 for v in movers), l  # passes with no, one, two, three and four movers
