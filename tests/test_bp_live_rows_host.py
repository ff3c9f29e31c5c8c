"""csrc/bp_masks.h, the part of the live-rows logic that is plain C++: bp_row_dead (which window rows the one-workgroup sort leaves
out of a tile's list) and bp_part_rows (the rows of a (tile, part) wavefront of the walks, cut at the list's live end), compiled
for the host and compared with their definitions - at the batch boundary (63 / 64 / 65 live rows), the count walk's part boundary
(255 / 256 / 257), an empty list, and parts the host's upper bound made room for that no live row reaches."""
import ctypes
import os
import subprocess

from conftest import ROOT


def _lib(tmp_path):
    src = tmp_path / "live.cpp"
    src.write_text('#include "bp_masks.h"\n'
                   'extern "C" int dead(int end, int p_first) { return bp_row_dead(end, p_first) ? 1 : 0; }\n'
                   'extern "C" void part_rows(uint32_t off, uint32_t n_live, uint32_t q, uint32_t part, uint32_t* j) { bp_part_rows(off, n_live, q, part, j[0], j[1]); }\n')
    lib = tmp_path / "live.so"
    subprocess.check_call(["g++", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "smcounter_amd", "csrc"), "-o", str(lib), str(src)])
    L = ctypes.CDLL(str(lib))
    L.dead.argtypes = [ctypes.c_int, ctypes.c_int]
    L.part_rows.argtypes = [ctypes.c_uint32] * 4 + [ctypes.POINTER(ctypes.c_uint32)]
    return L


def test_a_row_is_dead_when_it_ends_at_or_before_the_tiles_first_position(tmp_path):
    """`end` is exclusive: an alignment with end == p_first + 1 covers the tile's first locus, one with end == p_first covers none
    of the tile's - the walks' own overlap test is end > p_first (bp_walk_batch, bp2_cover64)."""
    L = _lib(tmp_path)
    for p_first in (0, 1, 63, 64, 1000, 2**31 - 2):
        for end in (p_first - 150, p_first - 1, p_first, p_first + 1, p_first + 64, p_first + 150):
            if -2**31 <= end < 2**31:
                assert bool(L.dead(end, p_first)) == (end <= p_first), (end, p_first)


def test_the_parts_of_a_list_end_at_its_live_rows(tmp_path):
    L = _lib(tmp_path)
    j = (ctypes.c_uint32 * 2)()
    for part in (64, 256, 4096):
        for window in (0, 1, 63, 64, 65, 255, 256, 257, 513, 4500, 16384):
            for n_live in sorted({0, 1, 63, 64, 65, 255, 256, 257, window // 2, window} & set(range(window + 1))):
                for off in (0, 7, 123456789):
                    n_parts = (window + part - 1) // part                      # the host's grid: from the window, not from the live rows
                    covered = 0
                    for q in range(n_parts):
                        L.part_rows(off, n_live, q, part, j)
                        j0, j1 = int(j[0]), int(j[1])
                        assert j0 == off + q * part
                        if q * part < n_live:
                            assert j1 == off + min(n_live, (q + 1) * part) and j1 > j0
                            covered += j1 - j0
                        else:
                            assert j0 >= j1, "a part behind the live rows must be empty"
                    assert covered == n_live
