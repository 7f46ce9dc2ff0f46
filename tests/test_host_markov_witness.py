"""The host's KmerMarkovModel / PosMarkovModel (portcullis_amd/host/include/portcullis/ml/markov_model.hpp) against what the
reference's own lib/src/markov_model.cc trained and scored (tests/golden/markov, made by tests/golden/make_markov_fixture.py, whose
docstring lists the cases).  tests/cpp/markov_witness_check.cc is the witness program over the project's header: it reads the same
training and query strings, which this test cuts again from the seeds, and prints every size after training, every size after
scoring and every score.  The program is host code with a main of its own, built with the address and undefined-behaviour
sanitizers linked in, and run directly: no context, no GPU.  Sizes, sentinels and the scores of all-ones products are exact; every
other score is within 1e-12 * max(1, |x|)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_markov_fixture as fx  # noqa: E402  (genomes, junctions, windows; it touches nothing on import)


def test_host_models_match_the_witness(tmp_path):
    exe, text = str(tmp_path / "markov_witness_check"), str(tmp_path / "in.txt")
    subprocess.check_call(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g", "-std=c++17", "-Wall",
                           f"-I{ROOT}/portcullis_amd/host/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "markov_witness_check.cc")])
    with open(text, "w") as f:
        f.write(fx.witness_input(fx.genomes(), fx.CASES))
    out = subprocess.run([exe, text], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert out.returncode == 0 and "runtime error" not in out.stderr, out.stdout[-2000:] + out.stderr[-4000:]
    got = fx.parse_output(out.stdout)
    want = fx.load_cases()
    assert list(got) == [w["name"] for w in want]
    for w in want:
        g, bits = got[w["name"]], fx.load_bits(w["name"])
        assert g["trained"] == w["trained"], (w["name"], g["trained"], w["trained"])
        assert g["scored"] == w["scored"], (w["name"], g["scored"], w["scored"])
        assert g["bits"].shape == bits.shape and ((g["bits"] == fx.NOT_ASKED) == (bits == fx.NOT_ASKED)).all(), w["name"]
        asked = bits != fx.NOT_ASKED
        a, b = g["bits"].view(np.float64), bits.view(np.float64)
        exact = asked & ((b == 0.0) | (b == -300.0) | (b == -100.0))
        assert (g["bits"][exact] == bits[exact]).all(), w["name"]
        assert (np.abs(a[asked] - b[asked]) <= 1e-12 * np.maximum(1.0, np.abs(b[asked]))).all(), (w["name"], np.abs(a[asked] - b[asked]).max())
