"""Build-time check of fb_coop_kernel's gfx950 code: the launch bound of every instantiation (kernels_fbcoop.h: FbCoopBounds) is
chosen so that its rows fit the VGPRs that bound leaves — a spilled row is reloaded in every step of the sweep."""
import pytest

from test_isa_budget import _body, _scratch, isa  # noqa: F401  (the listing fixture)


@pytest.mark.parametrize("name", ["_Z14fb_coop_kernelILi7ELb0EEv8FbParams", "_Z14fb_coop_kernelILi4ELb0EEv8FbParams",
                                  "_Z14fb_coop_kernelILi7ELb1EEv8FbParams", "_Z14fb_coop_kernelILi4ELb1EEv8FbParams",
                                  "_Z14fb_coop_kernelILi1ELb0EEv8FbParams", "_Z14fb_coop_kernelILi1ELb1EEv8FbParams"])
def test_cooperative_row_block_kernels_do_not_spill(isa, name):  # noqa: F811
    body = _body(isa, name)
    assert not _scratch(body), name
    assert sum(1 for l in body if l.strip().startswith("s_barrier")) >= 3, "the macro-step barriers are expected in the kernel"
