"""The method of the scripts/*_ab.py, stated once: two (or more) legs of one workload in ONE process and one build, under one
stated GPU_MAX_HW_QUEUES, on synthetic CKD tables; a warm-up of every leg, the bitwise comparison of what the legs return, then
the legs alternating (a 1, b 1, a 2, ...), every pass printed, and per leg the sorted rates, the median and the spread
(max - min).  Report keeps the printed lines for --out.  Each script states its legs, its sizes and what is its own."""
import argparse
import contextlib
import importlib
import os
import sys
import tempfile
from statistics import median

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "scripts"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

QUEUES = "GPU_MAX_HW_QUEUES"


def queues(value):
    """The hardware queues of this process, before the first import that touches the GPU or sets the variable: a value of the
    environment holds; without one, `value` ("4": the runtime's default, "16": what hyperspectral_bench and
    spectrum_levels_bench set) or, with None, no setting at all.  Returns what holds, for the header line."""
    if value is not None:
        os.environ.setdefault(QUEUES, value)
    elif QUEUES not in os.environ:
        import hyperspectral_bench, spectrum_levels_bench     # both default the variable on import: let them now, and undo it
        os.environ.pop(QUEUES, None)
    return os.environ.get(QUEUES)


def parser(out=None):
    """The arguments every A/B takes; `out`: the default of --out (None: print only)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--out", default=out, help="also write the printed lines to this file")
    return ap


def package():
    return importlib.import_module("radiativetransfer-sos_amd")


def synthetic_tables(link_aerosols=False):
    """Synthetic CKD tables (scripts/synth_ckd.py) in a temporary directory that becomes SOS_ABS_ROOT; link_aerosols: with the
    aerosol tables of the WMO / Shettle & Fenn models next to them."""
    import synth_ckd
    root = tempfile.mkdtemp(prefix="synth_fic_")
    synth_ckd.write_tables(root)
    if link_aerosols:
        import hyperspectral_bench
        hyperspectral_bench.link_aerosol_tables(root)
    os.environ["SOS_ABS_ROOT"] = root
    return root


class Report:
    """say() prints a line at once and keeps it; close() writes the lines to `out` if one was given."""

    def __init__(self, out=None):
        self.out, self.lines = out, []

    def say(self, text):
        print(text, flush=True)
        self.lines.append(text)

    def close(self):
        if self.out:
            os.makedirs(os.path.dirname(os.path.abspath(self.out)), exist_ok=True)
            with open(self.out, "w") as f:
                f.write("\n".join(self.lines) + "\n")


@contextlib.contextmanager
def switch(name, on):
    """A leg under the environment switch `name` (SOS_SPECTRUM_*_PER_CALL): "1" if on, unset if not; as before on exit."""
    was = os.environ.get(name)
    if on:
        os.environ[name] = "1"
    else:
        os.environ.pop(name, None)
    try:
        yield
    finally:
        if was is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = was


def tuples_identical(a, b):
    """Two results equal bit for bit (np.array_equal per array): lists or tuples nested to any depth, of equal lengths."""
    if isinstance(a, (list, tuple)) or isinstance(b, (list, tuple)):
        return (isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)) and len(a) == len(b) and
                all(tuples_identical(x, y) for x, y in zip(a, b)))
    return bool(np.array_equal(np.asarray(a), np.asarray(b)))


def warm_up(rs, kw):
    """One sos_proc: library load, surface matrices, caches.  The scripts follow it with one pass of every leg."""
    import torch
    rs.sos_proc(**kw)
    torch.cuda.synchronize()


def one_pass(leg, name, rate_unit):
    """--one-leg: a warm-up pass (tables parsed, caches filled) and a single pass of one leg, for a kernel trace."""
    leg()
    print("[%s] %.1f %s" % (name, leg()[0], rate_unit), flush=True)


def host_phases(njobs, per):
    """A per_pass of alternate() for legs whose extra is the timings dictionary of a pass."""
    def fmt(tm):
        return "host phases per %s (ms): %s" % (per, ", ".join("%s %.4f" % (q, 1e3 * v / njobs) for q, v in tm.items()))
    return fmt


def alternate(legs, runs, rate_unit, say, per_pass=None):
    """legs: name -> callable returning (rate, extra), in the order of a round.  `runs` rounds, one line per pass
    (per_pass(extra) adds a script's own columns), then per leg the sorted rates, the median and max - min.
    Returns ({name: rates}, {name: extras}), both in the order of the passes."""
    width = max(len(name) for name in legs)
    rates, extras = {name: [] for name in legs}, {name: [] for name in legs}
    for k in range(runs):
        for name, leg in legs.items():
            rate, extra = leg()
            rates[name].append(rate)
            extras[name].append(extra)
            say("[%-*s %d] %8.1f %s%s" % (width, name, k + 1, rate, rate_unit, "   " + per_pass(extra) if per_pass else ""))
    for name, v in rates.items():
        say("%s  %-*s: %s   median %.1f, max - min %.1f" % (
            rate_unit, width, name, " ".join("%.1f" % x for x in sorted(v)), median(v), max(v) - min(v)))
    return rates, extras


def job_cost(rates, base, leg, what, per, say):
    """What leg `leg` costs over leg `base` per job, from the medians of their rates (jobs per second)."""
    lo, hi = 1e3 / median(rates[base]), 1e3 / median(rates[leg])
    say("cost of %s per %s, from the medians: %.4f ms (%.4f -> %.4f ms per job)" % (what, per, hi - lo, lo, hi))


def phase_medians(extras, njobs, per, say, keys=None):
    """Per leg the median over the passes of each host phase (keys None: those of the first pass), in ms per job."""
    width = max(len(name) for name in extras)
    for name, v in extras.items():
        say("median host phase per %s (ms)  %-*s: %s" % (per, width, name, ", ".join(
            "%s %.4f" % (q, 1e3 * median(t.get(q, 0.0) for t in v) / njobs) for q in (keys or v[0]))))
