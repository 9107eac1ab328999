"""The long form of the record store on every path it takes, on MI355X (tests/_relax_long.py): the field widths (distances with an upper
half of 0, 1 and >= 2, columns at and beyond 0x1fff / 0x8000, entry positions beyond 16 bits, MPC_RL_MAXLEN and the fall to the gather
layout one position later), the grid-stride trips of var_build_long_kernel, split ranges before a commit, batched and wide joins,
and form changes on one context. Everything 0 ulp against the CPU oracle; every case asserts its route from mpcgpu_relax_info. What
the inputs hold is asserted in tests/test_relax_long_table.py, whose counts are repeated here. Partial stores and stores in
segments of the long form: tests/test_gpu_store_segments.py."""
import pytest
import torch

import _relax_long as L

pytestmark = pytest.mark.gpu


def test_long_dist_hi():
    """9000 positions, three low-complexity stretches, no knob. First blocks by dist.hi: 1186 rows with 0, 159 with 1, 155 with >= 2
    (all with lo != 0); columns: 96 equal to 0x1fff, 1845 in (0x1fff, 0x7fff]; 1404 rows of three and more blocks; largest record
    11 130 blocks. The join by rows has C2 = 600 on a long store, where the host code launches build_post_rows_long_kernel<16>; the
    launch counters (1/0/0: the row form) do not tell <8> from <16>, so the width is asserted and the kernel follows from it"""
    L.check_field("dist_hi")


def test_long_col_high():
    """40 000 positions: 952 stored columns above 0x8000 (39 900 ..), 952 entry positions >= 65 536; largest record 40 417 blocks"""
    L.check_field("col_high")


def test_long_col_8000():
    """33 000 positions, a stretch across column 32 768: 10 columns equal to 0x7fff, 10 equal to 0x8000, 272 in (0x1fff, 0x7fff], 259
    above 0x8000; 485 entry positions >= 65 536"""
    L.check_field("col_8000")


def test_long_maxlen():
    """65 534 = MPC_RL_MAXLEN positions (a glycine background with stretches at rows 100 and 65 480, tests/_relax_long.py says why)
    against 40, 55 and 30: band-long, is_fallback 0. 117 rows with dist.hi >= 2 (first blocks 65 000 blocks before their overflow
    blocks), 394 with 0; 1050 columns above 0x8000; 2867 entry positions >= 65 536; 479 rows of three and more blocks; largest
    record 66 271 blocks"""
    L.check_field("maxlen")


def test_long_dense_rows_fall_to_slabs():
    """65 534 positions of mixed composition: the reference keeps 2 327 847 of the 2 621 360 cells of 65 534 x 40, rows of 60 000
    entries; the store is band-long, the relax falls to the CSR slabs at the first iteration, values equal the oracle's"""
    L.check_dense()


def test_long_over_maxlen_falls_to_gather():
    """65 535 positions: stage A accepts it (its limit is 65 535 per sequence, mpcgpu_stage_a.inc), build_var_store does not
    (MPC_RL_MAXLEN): CSR slabs, relax_kernel, is_fallback 1, values equal the oracle's"""
    L.check_over()


def test_long_grid_stride():
    """n * n >= 8 x the CU count (46 sequences on 256 CUs): every workgroup of var_build_long_kernel builds a second record on its scratch"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = L.check_stride(cus)
    assert n * n > 4 * cus and n * n >= 2 * min(n * n, 4 * cus), (n, cus)


def test_long_ranges():
    """halves, an uneven split, the empty range, and a second iteration split differently from the first, before one commit each"""
    L.check_ranges()


def test_long_joins():
    """three joins in one batch (build_post_rows_batch_long_kernel<8>), weighted joins, MPCGPU_BP=rows against =sort, C2 > 512"""
    L.check_joins()


def test_long_form_changes():
    """short -> long -> short (smaller n) -> long (larger n) -> short on one context; relax_info as on fresh contexts"""
    L.check_forms("gpu")
