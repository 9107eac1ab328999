"""Build-time check of sw_kernel's gfx950 code (kernels_sw.h), from the listing's kernel metadata: no instantiation spills a
register or has a private segment."""
import re

from test_isa_budget import isa  # noqa: F401  (the listing fixture)

NAMES = ["_Z9sw_kernelILi%dELb0EEv8SwParams" % h for h in range(1, 9)] + ["_Z9sw_kernelILi8ELb1EEv8SwParams"]


def test_sw_kernel_has_no_spills_and_no_private_segment(isa):  # noqa: F811
    meta = isa[isa.index("amdhsa.kernels:"):]
    for name in NAMES:
        i = meta.index(".name:           " + name + "\n")  # (raises when the kernel is not in the listing)
        # a kernel's entry: from the list item before its name to the next list item
        start = meta.rindex("\n  - .", 0, i)
        end = meta.find("\n  - .", i)
        entry = meta[start:end if end > 0 else len(meta)]
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", entry).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", entry).group(1)) == 0, name
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1)) == 0, name
        if "ELb0E" in name:  # the sweeps of one row block: eight waves per SIMD
            assert int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1)) <= 64, name
