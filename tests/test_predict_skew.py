"""BISBM_PREDICT_SKEW on the CPU (csrc/bisbm_predict_skew.hpp).

The feeder wave of the production kernel predicts each step's inverse-CDF target a chunk ahead; the passes that read on the
prediction check it against their own scan, so any prediction gives the same chain.  BISBM_PREDICT_SKEW = n makes misses happen:
every n-th step of a chunk is handed the next block.  tests/native/predict_skew_check.cpp includes the header the host side and
the kernel include: unset, empty and 0 leave SweepParams::predict_skew at its default 0, under which no prediction changes; with
n > 0 exactly the steps n - 1 modulo n get another block, always in range.  Built with the address and undefined-behaviour
sanitizers: a plain program, CPU only.  (The chains themselves: test_gpu_quad32_predicted_target.py.)"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_skew_defaults_and_arithmetic(tmp_path):
    exe = str(tmp_path / "predict_skew_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                    "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "predict_skew_check.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    c = {k: int(v) for k, v in re.findall(r"([a-z_]+) (\d+)", r.stdout.splitlines()[-1])}
    assert c["cases"] > 100000 and c["wrong"] == 0 and c["skewed"] > 0, r.stdout


def test_the_host_reads_the_variable_into_the_launch_parameters():
    src = open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "csrc", "bisbm_anneal.hip")).read()
    assert 'p.predict_skew = predict_skew_from_env(getenv("BISBM_PREDICT_SKEW"));' in src
