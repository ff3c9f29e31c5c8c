"""What the pages of --spikeScanFilter must hold, restated from the columns a replicate page prints: shared by the tests without a GPU
(hand-made replicates) and the command-line test on the GPU (the replicates of the passes' own runs).  A replicate is a pair (FILTER
column, CALLED column) of a .spikeAF*.replicates.txt line."""
from smcounter_amd import dsaf

NAMES = ("LM", "LSM", "HP", "LowC", "DP", "SB", "LowQ", "R1CP", "R2CP", "PrimerCP", "RepT", "RepS", "SL", "Other_Repeat")
HEADER = ("CHROM", "POS", "REF", "ALT", "TARGET", "REPS", "CALLED", "PASS", "RATE_PASS", "LO95", "HI95") + NAMES


def counts(replicates):
    """-> (REPS, CALLED, PASS, per name the called replicates whose FILTER column holds it - once per replicate)."""
    called = [f for f, c in replicates if int(c) == 1]
    return len(replicates), len(called), sum(1 for f in called if f == "PASS"), [sum(1 for f in called if n in f.split(";")) for n in NAMES]


def line(head, replicates, cell=()):
    """The page's line as fields: head = [CHROM, POS, REF, ALT, TARGET]; cell: the axis column and MTDEPTH of a cell's page."""
    reps, called, passed, tally = counts(replicates)
    lo, hi = dsaf.wilson(passed, reps)
    return list(head) + list(cell) + ["%d" % reps, "%d" % called, "%d" % passed, dsaf.frac_text(float(passed) / reps), dsaf.frac_text(lo),
                                      dsaf.frac_text(hi)] + ["%d" % n for n in tally]


def curve_line(head4, n, targets, per_target):
    """[CHROM, POS, REF, ALT], N, RATE_PASS@ ascending, T95_PASS; per_target[t]: the replicates at targets[t]."""
    rates = []
    for reps in per_target:
        r, _, p, _ = counts(reps)
        rates.append(float(p) / r)
    best = dsaf.t95(targets, rates)
    order = sorted(range(len(targets)), key=lambda t: targets[t])
    return list(head4) + ["%d" % n] + [dsaf.frac_text(rates[t]) for t in order] + ["NA" if best is None else "%g" % best]


def check_bedgraphs(prefix, targets, loci, page, curve):
    """The bedgraphs follow from the pages.  loci: every (chrom, pos) of the target in order; page / curve: the two pages' lines as
    fields, headers included."""
    i_rate, i_t95 = page[0].index("RATE_PASS"), curve[0].index("T95_PASS")
    scanned = [(f[0], int(f[1])) for f in curve[1:]]
    for t in targets:
        got = open("%s.spikeScan%g.passrate.bedgraph" % (prefix, t)).read().splitlines()
        mine = [f for f in page[1:] if f[4] == "%g" % t]
        assert got == ["%s\t%d\t%d\t%s" % (f[0], int(f[1]) - 1, int(f[1]), f[i_rate]) for f in mine] and len(mine) == len(scanned)
    t95 = {(f[0], int(f[1])): f[i_t95] for f in curve[1:]}
    got = open(prefix + ".spikeScan.t95pass.bedgraph").read().splitlines()
    assert got == ["%s\t%d\t%d\t%s" % (c, p - 1, p, "1" if t95.get((c, p), "NA") == "NA" else t95[(c, p)]) for c, p in loci]
    return got
