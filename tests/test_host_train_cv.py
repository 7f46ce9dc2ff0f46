"""`portcullis_amd train --folds` where it needs no device: its help and every refusal, with the devices hidden (in the manner of
tests/test_host_forest_save.py).  All of them come before a device is opened; "No MI355X" stays the last refusal."""
import os
import subprocess

from filt_cases import build_cases, tab_of

import cv_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")
NO_DEVICE = "No MI355X (HIP device) is visible"


def train(*args):
    """the program with the devices hidden: nothing here may open one"""
    assert os.path.exists(EXE), f"{EXE} missing: run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PORTCULLIS_", "PJB_"))}
    env["HIP_VISIBLE_DEVICES"] = env["ROCR_VISIBLE_DEVICES"] = "-1"
    return subprocess.run([EXE, "train", *args], capture_output=True, text=True, timeout=60, env=env)


def test_help_lists_the_new_options():
    p = train("--help")
    assert p.returncode == 1
    for text in ("-k [ --folds ] arg (=0)", "--threshold arg (=0.5)", "<prefix>.cv_results", "<prefix>.cv_scores", "Not with --markov"):
        assert text in p.stdout, text
    not_built = p.stdout[p.stdout.index("Not built:"):]
    assert "variable importance" in not_built and "out-of-bag" in not_built and "--fraction" in not_built


def test_refusals_with_the_devices_hidden(tmp_path):
    case = sorted(build_cases().items())[0][1]
    lines = tab_of(case).split("\n")
    head, rows = lines[0], [l for l in lines[1:] if l]
    assert len(rows) >= 6
    prep = tmp_path / "prep"
    prep.mkdir()
    (prep / "portcullis.genome.fa").write_text(">unused\nACGT\n")

    def tab(name, some):
        (tmp_path / name).write_text("\n".join([head] + some) + "\n")
        return str(tmp_path / name)

    pos, neg = tab("pos.tab", rows[::2]), tab("neg.tab", rows[1::2])
    out = str(tmp_path / "out" / "model")

    def refused(p, *texts):
        assert p.returncode == 4, (p.returncode, p.stdout[-500:], p.stderr[-500:])
        for t in texts:
            assert t in p.stderr, (t, p.stderr)
        assert NO_DEVICE not in p.stderr or NO_DEVICE in texts[0]
        for ext in (".forest", ".cv_results", ".cv_scores"):
            assert not os.path.exists(out + ext)

    refused(train("-o", out, "--folds", "1", str(prep), pos, neg), "--folds must be 0 (no cross-validation) or at least 2: 1")
    refused(train("-o", out, "-k", "-3", str(prep), pos, neg), "--folds must be 0 (no cross-validation) or at least 2: -3")
    refused(train("-o", out, "--folds", str(len(rows) + 1), str(prep), pos, neg), f"--folds {len(rows) + 1} is more than the {len(rows)} junctions")
    for t in ("-0.01", "1.5", "nan"):
        refused(train("-o", out, "--folds", "2", "--threshold", t, str(prep), pos, neg), "--threshold must lie between 0 and 1")
    refused(train("-o", out, "--folds=3", "--markov", str(prep), pos, neg), "--folds cannot be combined with --markov",
            "the Markov models would have seen the held-out junctions", "fold by fold is not built")
    # a fold that would train on one label only: one negative junction, so the fold that holds it out trains on positives alone.
    # The table's order is the sorted order here, so the fold is cv_model's for that junction's place
    one = tab("one.tab", rows[3:4])
    most = tab("most.tab", rows[:3] + rows[4:])
    fold = int(cm.assign_folds(len(rows), 3, 1236456789)[3]) + 1
    refused(train("-o", out, "--folds", "3", str(prep), most, one),
            f"Fold {fold} of 3 would train on positive junctions only ({len(rows) - list(cm.assign_folds(len(rows), 3, 1236456789)).count(fold - 1)} junctions)")
    refused(train("-o", out, "--folds", "3", str(prep), one, most), f"Fold {fold} of 3 would train on negative junctions only")
    # what is in order reaches the device refusal, as before and as the last one
    for args in (("--folds", "0"), (), ("--folds", "3"), ("-k", "2", "--threshold", "0"), ("--folds", "2", "--threshold=1")):
        refused(train("-o", out, *args, str(prep), pos, neg), NO_DEVICE, "no CPU fallback")
    refused(train("-o", out, "--folds", "0", "--markov", str(prep), pos, neg), NO_DEVICE)
