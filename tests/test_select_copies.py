"""smc_select_alignments_copies without a GPU: the entry is declared, bound and additive (ABI 11), its limit is the wrapper's, and
devplanes.select_copies refuses a batch it cannot hand on before it touches the device."""
import os
import re

import pytest

from conftest import ROOT
from smcounter_amd import _lib, devplanes


def _header():
    return open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()


def test_the_entry_is_declared_and_bound_at_abi_11():
    h = _header()
    assert re.search(r"^#define SMC_ABI_VERSION 11$", h, re.M)
    m = re.search(r"\bint\s+smc_select_alignments_copies\s*\(([^;]*)\);", h)
    assert m
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 18 and args[0] == "smc_ctx* ctx" and args[2] == "int64_t aln_stride_bytes" and args[-1] == "void* stream"
    assert "smc_select_alignments_copies" in _lib.SYMBOLS
    L = _lib.load()
    assert len(L.smc_select_alignments_copies.argtypes) == 18
    # (additive: the single call keeps its signature)
    assert len(L.smc_select_alignments.argtypes) == 16 and len(L.smc_select_alignments_keyed.argtypes) == 19


def test_the_limit_is_the_headers():
    m = re.search(r"^#define SMC_SEL_MAX_SELECTIONS (\d+)$", _header(), re.M)
    assert m and int(m.group(1)) == devplanes.SEL_MAX_SELECTIONS == 2048


class _Run(object):
    def __init__(self, ptr, n):
        self.n_aln, self.aln = n, self
        self._p = ptr

    def data_ptr(self):
        return self._p


@pytest.mark.parametrize("runs, seeds, fracs", [
    ([], [], [0.5]),                                                            # no copy
    ([_Run(0, 4)], [1], []),                                                    # no fraction
    ([_Run(0, 4)] * 2, [1], [0.5]),                                             # a seed short
    ([_Run(0, 4)] * 64, list(range(64)), [0.5] * 33),                           # 2112 selections
    ([_Run(0, 4), _Run(256, 4), _Run(768, 4)], [1, 2, 3], [0.5]),               # no constant stride
    ([_Run(0, 4), _Run(256, 5)], [1, 2], [0.5]),                                # copies of two lengths
])
def test_select_copies_refuses_before_the_device(runs, seeds, fracs):
    with pytest.raises(ValueError, match="select_copies"):
        devplanes.select_copies(None, runs, dict(nl=8, n_bc=2, n_pair=2, status=0), 0, [1, 2], seeds, fracs)
