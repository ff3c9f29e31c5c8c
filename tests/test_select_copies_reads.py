"""smc_select_alignments_reads_copies without a GPU: the entry is declared, bound and additive (ABI 11), and
devplanes.select_copies_reads refuses a batch it cannot hand on before it touches the device."""
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
    m = re.search(r"\bint\s+smc_select_alignments_reads_copies\s*\(([^;]*)\);", h)
    assert m
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 20 and args[0] == "smc_ctx* ctx" and args[2] == "int64_t aln_stride_bytes" and args[-1] == "void* stream"
    assert args[10:15] == ["const uint32_t* d_masks", "int64_t mask_words", "int64_t mask_copy_stride_words", "int32_t n_masks", "int64_t n_ids"]
    # (declared behind the barcode-level batch)
    assert h.index("int smc_select_alignments_copies(") < h.index("int smc_select_alignments_reads_copies(")
    assert "smc_select_alignments_reads_copies" in _lib.SYMBOLS
    L = _lib.load()
    assert len(L.smc_select_alignments_reads_copies.argtypes) == 20
    # (additive: the other selections keep their signatures)
    assert len(L.smc_select_alignments.argtypes) == 16 and len(L.smc_select_alignments_keyed.argtypes) == 19
    assert len(L.smc_select_alignments_copies.argtypes) == 18


class _Run(object):
    def __init__(self, ptr, n):
        self.n_aln, self.aln = n, self
        self._p = ptr

    def data_ptr(self):
        return self._p


@pytest.mark.parametrize("runs, n_masks", [
    ([], 2),                                                                    # no copy
    ([_Run(0, 4)], 0),                                                          # no mask
    ([_Run(0, 4)] * 64, 33),                                                    # 2112 selections
    ([_Run(0, 4), _Run(256, 4), _Run(768, 4)], 1),                              # no constant stride
    ([_Run(0, 4), _Run(256, 5)], 1),                                            # copies of two lengths
])
def test_select_copies_reads_refuses_before_the_device(runs, n_masks):
    with pytest.raises(ValueError, match="select_copies_reads"):
        devplanes.select_copies_reads(None, runs, dict(nl=8, n_bc=2, n_pair=2, status=0), 0, 4096, 1, 0, n_masks)
