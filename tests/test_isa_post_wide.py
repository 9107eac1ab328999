"""Build-time check of post_wide_kernel's gfx950 code (kernels_postw.h): a workgroup of 1024 threads is 16 waves, four per SIMD, which
leaves each 128 VGPRs; and nothing of it may live in scratch memory."""
import re

from test_isa_budget import _body, _scratch, isa  # noqa: F401  (the listing fixture)

NAME = "_Z16post_wide_kernel14PostWideParams"


def test_post_wide_kernel_fits_sixteen_waves(isa):  # noqa: F811
    body = _body(isa, NAME)  # (raises when the kernel is not in the listing)
    assert not _scratch(body), "scratch accesses in post_wide_kernel"
    i = isa.index(".amdhsa_kernel " + NAME)
    desc = isa[i:isa.index(".end_amdhsa_kernel", i)]
    vgprs = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", desc).group(1))
    assert vgprs <= 128, vgprs
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1)) == 0
