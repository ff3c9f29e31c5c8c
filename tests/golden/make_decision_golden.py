"""Generate tests/golden/decision/<family>.npz (BUILD CONTAINER ONLY, like make_golden.py).

Runs the reference implementation itself (through oracle/ref_harness.py) on the constructed loci of tests/decision_cases.py and stores,
in make_golden.emit()'s format, the pileup, the fake FASTA, the parameters and per locus what the reference returned - now with `final`,
the (key, PI) items of finalDict in the order the emulated Python 2 dict hands them to sorted() (smCounter.py:534) - plus, per locus,
the label, the design of a gate locus and an `order_class` computed from the reference's OWN numbers in `final`:

  pinned        every pair of keys whose order decides maxBase / secondMaxBase is either bit-equal in the reference's doubles or further
                apart than 1e-6 relative (the project's PI tolerance), the bit-equal ones are all A / T / G / C, and finalDict holds
                fixed keys only (A, T, G, C, N, DEL): the order of the tied keys is the slot order of those keys, whatever their
                insertion history;
  pinned_indel  the same, but finalDict holds an indel key: its hash may take a base's slot, so the expected order is the one the
                harness's Py2Dict recorded in `final`;
  unpinned      everything else: a tie that involves N, DEL or an indel key, or a difference below 1e-6 that is not bit-equal.

The files go to the SUBDIRECTORY on purpose: conftest.golden_files() globs tests/golden/*.npz, and these loci have tests of their own
(tests/test_decision_ref.py, tests/test_gpu_decision.py).
Usage:  PYTHONHASHSEED=0 python tests/golden/make_decision_golden.py
"""
import dataclasses
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import decision_cases  # noqa: E402
from decision_cases import FAMILIES, check_fixture, order_class  # noqa: E402

OUT = os.path.join(HERE, "decision")
SIZE_CAP = 700000        # below the largest pileup golden committed (stress4.npz)


def emit(name):
    import ref_harness
    from smcounter_amd import pileup
    pb, chroms, params, labels, designs = getattr(decision_cases, name)()
    res = [{k: v for k, v in r.items() if k != "pileup"} for r in ref_harness.run_reference(pb, params, chroms)]
    assert not any(r["row"].startswith("Exception thrown!") for r in res), name
    classes = [order_class(r["final"]) for r in res]
    path = os.path.join(OUT, name + ".npz")
    pileup.save_npz(path, pb, params=dataclasses.asdict(params), chroms=chroms, expected=res, labels=labels, designs=designs,
                    order_class=classes)
    print("%-11s %4d loci %7d reads %7d bytes  %s" % (name, pb.n_loci, pb.n_reads, os.path.getsize(path),
                                                      "  ".join("%d %s" % (classes.count(c), c) for c in sorted(set(classes)))))
    for lab, c in zip(labels, classes):
        if c == "unpinned" or (name != "ties_indel" and c != "pinned"):
            print("    %-9s %s" % (c, lab))
    assert os.path.getsize(path) < SIZE_CAP
    pb2, extra = pileup.load_npz(path)
    check_fixture(name, extra)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    for family in FAMILIES:
        emit(family)
