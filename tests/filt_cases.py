"""The inputs of the filt rule witness (tests/golden/make_rule_filter_fixture.py, test_host_filt.py): the cases of the junctools witness and a
wider fuzz set of a few hundred junctions on three targets.  tab_of() is the oracle's .junctions.tab of a case: the table the rules run over."""
from fuzzgen import make_reads, to_batch
from junctools_cases import build_cases as junctools_build_cases


def build_cases():
    cases = junctools_build_cases()
    contigs = []
    for tid, seed in enumerate((31, 32, 33)):
        genome, rr = make_reads(seed, n_reads=4000, paired=True, glen=100000 + 5000 * tid, n_tx=50)
        for r in rr:
            r["tid"] = tid
            if r.get("mtid", -1) >= 0:
                r["mtid"] = tid
        contigs.append((f"ctg{tid + 1}", genome, rr))
    cases["fuzz_wide_FR"] = ([(n, len(g)) for n, g, _ in contigs], {t: g for t, (_, g, _) in enumerate(contigs)},
                             {t: to_batch(rr) for t, (_, _, rr) in enumerate(contigs)}, "FR")
    return cases


def tab_of(case):
    from oracle import oracle as orc
    refs, genomes, batches, orientation = case
    rows, _ = orc.run_prep_like(refs, genomes, batches, orientation)
    return orc.write_tab(rows, [n for n, _ in refs], [l for _, l in refs]).decode()
