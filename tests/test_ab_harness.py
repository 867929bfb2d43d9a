"""scripts/ab_harness.py: the order of the passes, the figures of the summary, the --out file, the environment switch and the
bitwise comparison (no GPU, no process)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import ab_harness as ab

RATES = {"a": [10.0, 30.0, 20.0, 60.0], "b": [5.0, 1.0, 3.0, 2.0]}


@pytest.mark.parametrize("runs,medians,spreads", [(3, (20.0, 3.0), (20.0, 4.0)), (4, (25.0, 2.5), (50.0, 4.0))])
def test_alternate(tmp_path, runs, medians, spreads):
    calls = []

    def leg(name):
        def one():
            calls.append(name)
            k = calls.count(name) - 1
            return RATES[name][k], {"phase": 0.5 * (k + 1)}
        return one

    out = tmp_path / "sub" / "ab.txt"
    rep = ab.Report(str(out))
    rates, extras = ab.alternate({"a": leg("a"), "b": leg("b")}, runs, "things/s", rep.say, per_pass=lambda e: "phase %.1f" % e["phase"])
    assert calls == ["a", "b"] * runs
    assert rates == {name: v[:runs] for name, v in RATES.items()}
    assert extras["b"] == [{"phase": 0.5 * (k + 1)} for k in range(runs)]
    passes, summary = rep.lines[:2 * runs], rep.lines[2 * runs:]
    assert [ln.split("]")[0] for ln in passes] == ["[%s %d" % (name, k + 1) for k in range(runs) for name in "ab"]
    assert all("things/s" in ln for ln in passes) and passes[2].endswith("phase 1.0") and "%8.1f" % RATES["a"][1] in passes[2]
    assert len(summary) == 2
    for ln, name, med, spread in zip(summary, "ab", medians, spreads):
        assert ln.startswith("things/s  %s: " % name)
        assert " ".join("%.1f" % x for x in sorted(RATES[name][:runs])) in ln
        assert ln.endswith("median %.1f, max - min %.1f" % (med, spread))
    assert not out.exists()
    rep.close()
    assert out.read_text() == "\n".join(rep.lines) + "\n" and len(rep.lines) == 2 * runs + 2


def test_report_without_out_only_prints(capsys):
    rep = ab.Report()
    rep.say("one line")
    rep.close()
    assert capsys.readouterr().out == "one line\n" and rep.lines == ["one line"]


def test_phase_medians_and_job_cost():
    lines = []
    extras = {"flux": [{"trphi": 2.0, "finish": 1.0}, {"trphi": 4.0, "finish": 3.0}, {"trphi": 9.0, "finish": 2.0}],
              "split": [{"trphi": 1.0}, {"trphi": 1.0}, {"trphi": 7.0}]}
    ab.phase_medians(extras, 1000, "job", lines.append, keys=("trphi", "finish"))
    assert lines == ["median host phase per job (ms)  flux : trphi 4.0000, finish 2.0000",
                     "median host phase per job (ms)  split: trphi 1.0000, finish 0.0000"]
    del lines[:]
    ab.job_cost({"flux": [100.0, 50.0, 200.0], "split": [80.0, 20.0, 40.0]}, "flux", "split", "the split", "job", lines.append)
    assert lines == ["cost of the split per job, from the medians: 15.0000 ms (10.0000 -> 25.0000 ms per job)"]


def test_switch_restores(monkeypatch):
    name = "SOS_SPECTRUM_TEST_PER_CALL"
    monkeypatch.setenv(name, "before")
    with ab.switch(name, False):
        assert name not in os.environ
    assert os.environ[name] == "before"
    with ab.switch(name, True):
        assert os.environ[name] == "1"
    assert os.environ[name] == "before"
    monkeypatch.delenv(name)
    with ab.switch(name, True):
        assert os.environ[name] == "1"
    assert name not in os.environ
    with pytest.raises(RuntimeError):
        with ab.switch(name, True):
            raise RuntimeError("the leg failed")
    assert name not in os.environ


def test_queues(monkeypatch):
    monkeypatch.delenv(ab.QUEUES, raising=False)
    assert ab.queues("4") == "4" and os.environ[ab.QUEUES] == "4"
    assert ab.queues("16") == "4"                              # a value that is there holds
    monkeypatch.delenv(ab.QUEUES)
    assert ab.queues(None) is None and ab.QUEUES not in os.environ     # not even the default of the bench modules
    monkeypatch.setenv(ab.QUEUES, "8")
    assert ab.queues(None) == "8" and os.environ[ab.QUEUES] == "8"


def test_tuples_identical():
    a = [(np.arange(6.0).reshape(2, 3), 3, np.float64(0.1)), (np.ones(4), 2, np.float64(0.3))]
    b = [tuple(np.copy(x) for x in t) for t in a]
    assert ab.tuples_identical(a, b) and ab.tuples_identical([a, a], [b, b])
    b[1] = (b[1][0], b[1][1], np.nextafter(b[1][2], 1.0))                          # one bit
    assert not ab.tuples_identical(a, b) and not ab.tuples_identical([a, a], [a, b])
    assert not ab.tuples_identical(a, a[:1]) and not ab.tuples_identical(a[0], a[0][:2])
    assert not ab.tuples_identical(a[0], np.arange(3.0)) and not ab.tuples_identical(np.zeros(3), np.zeros(4))
