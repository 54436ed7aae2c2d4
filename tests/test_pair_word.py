"""The pair word of the four-steps pass on verified predictions (csrc/bisbm_pair_word.hpp) on the CPU.

In the one-stage kernels a row of step_quad32 is committed only if its scan found the target the feeder wave predicted, so the
feeder knows every input of a pair's clash test but the later step's margins and hands the rest over as one 10-bit field per
pair: k and which margin to ask.  The field and its test are plain C++ in a header the kernel includes;
tests/native/pair_word_check.cpp includes the same header and requires pair_clash<D>(pair_word_field(..), margins) ==
shared | column_clash<D>(..) for every r_i, s_i, r_j, s_j < 32, k in {0, 1, 2, 85, 86, 255}, margins at (D - 1) k - 1, (D - 1) k,
(D - 1) k + 1, 0, negative and past the cap in both halves of the packed word, D in {4, 8}, the field at each of the word's three
positions -- and that shared blocks, targets outside, kept and refused targets between, both boundary cases and k = 0 against a
negative margin all occurred.  Built with the address and undefined-behaviour sanitizers: a plain program, CPU only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_pair_word_is_the_pair_test(tmp_path):
    exe = str(tmp_path / "pair_word_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                    "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "pair_word_check.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("D ")]
    assert [l.split(":")[0] for l in lines] == ["D 4", "D 8"], r.stdout
    for l in lines:
        c = {k: int(v) for k, v in re.findall(r"([a-z_]+) (\d+)", l)}
        assert c["cases"] == 32 ** 4 * 6 * 12 and c["wrong"] == 0, l
        for name in ("shared", "outside", "between_kept", "between_refused", "kept_at_boundary", "refused_at_boundary", "zero_k_negative"):
            assert c[name] > 0, l
