"""The oracle's restatement of the filt stage's Markov models (kmm_* / pmm_* of oracle/portcullis_oracle.c) against what the
reference's own lib/src/markov_model.cc trained and scored (tests/golden/markov, made by tests/golden/make_markov_fixture.py, whose
docstring lists the cases): every size the oracle returns is the witness's size after training, and columns 11 to 13 of its feature
rows are the witness's scores, composed in the reference's order of operations.  Sizes, sentinels and the scores of all-ones products
are exact; every other score is within 1e-12 * max(1, |x|), which allows for one libm's log differing from another's."""
import os
import sys

import numpy as np
import pytest

from oracle import oracle as orc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_markov_fixture as fx  # noqa: E402  (genomes, junctions, windows; it touches nothing on import)

WITNESS = {c["name"]: c for c in fx.load_cases()}


@pytest.fixture(scope="module")
def genomes():
    return fx.genomes()


def test_fixture_covers_the_cases():
    assert [c["name"] for c in fx.CASES] == list(WITNESS)
    for case in fx.CASES:
        assert fx.load_bits(case["name"]).shape == (len(fx.case_rows(case)), 14)
    w = WITNESS["none_one_row"]           # an untrained position model: empty before a 24-base window is scored, 23 positions after
    assert w["trained"] == [0] * 8 and w["scored"][6:] == [23, 22]
    gate, counted = WITNESS["gate_skipped"], WITNESS["gate_counted"]
    assert gate["trained"][1] <= 36 < 1000 < counted["trained"][1]     # markov_model.cc:36: 65 539 and 65 542 bases are left out


@pytest.mark.parametrize("case", fx.CASES, ids=[c["name"] for c in fx.CASES])
def test_oracle_sizes_and_columns(case, genomes):
    w = WITNESS[case["name"]]
    bits = fx.load_bits(case["name"])
    idx = fx.case_rows(case)
    assert case["rows"] is None or not (case["cp"] or case["passing"] or case["failing"])   # the sets index the rows as they are passed
    rows = fx.junction_rows(orc.ROW_DTYPE, idx)
    F, M, _ = orc.filt_features([len(g) for g in genomes], dict(enumerate(genomes)), rows, [], case["cp"], case["passing"], case["failing"])
    got = [M["exon_size"], M["intron_size"], M["donor_pw_size"], M["acceptor_pw_size"]]
    assert got == [w["trained"][k] for k in (0, 1, 6, 7)], (got, w["trained"])
    for k, name in enumerate(fx.MODEL_NAMES):          # a model the witness left empty has an all-zero table
        if w["trained"][k] == 0:
            assert not M[name].any(), name
    want = fx.compose(case, bits, w["trained"], genomes)
    fx.assert_columns(np.ascontiguousarray(F[:, 11:14]), want, fx.exact_rows(bits), 1e-12)
