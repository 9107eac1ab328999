"""Build-time checks of the relax_band_kernel instantiations a store in segments launches (kernels_relaxb.h: MpcRbSegmented), the way
tests/test_isa_budget.py checks their unsegmented twins: the per-step base address must cost the walk neither a spill nor occupancy."""
import re

import pytest

from test_isa_budget import isa, _body, _scratch, _walk  # noqa: F401 (isa: the fixture)

TWINS = [("_Z17relax_band_kernelILi1024ELi15ELi2ELi0E14MpcRbSegmentedI11MpcRbWinAsmEEv15RelaxBandParams",
          "_Z17relax_band_kernelILi1024ELi15ELi2ELi0E11MpcRbWinAsmEv15RelaxBandParams", 15),
         ("_Z17relax_band_kernelILi1024ELi13ELi2ELi0E14MpcRbSegmentedI14MpcRbBlocksAsmEEv15RelaxBandParams",
          "_Z17relax_band_kernelILi1024ELi13ELi2ELi0E14MpcRbBlocksAsmEv15RelaxBandParams", 13)]
# the compiler's own code for the merge (MPCGPU_RELAX_MERGE=cxx): no hand-scheduled statements to count, the resources must match
CXX_TWINS = [("_Z17relax_band_kernelILi1024ELi15ELi2ELi0E14MpcRbSegmentedI11MpcRbWinCxxEEv15RelaxBandParams",
              "_Z17relax_band_kernelILi1024ELi15ELi2ELi0E11MpcRbWinCxxEv15RelaxBandParams"),
             ("_Z17relax_band_kernelILi1024ELi13ELi2ELi0E14MpcRbSegmentedI14MpcRbBlocksCxxEEv15RelaxBandParams",
              "_Z17relax_band_kernelILi1024ELi13ELi2ELi0E14MpcRbBlocksCxxEv15RelaxBandParams")]


def _resources(isa, name):
    get = lambda key: int(re.search(r"\.set %s\.%s, (\d+)" % (re.escape(name), key), isa).group(1))
    end = isa.index("; -- End function", isa.index("\n" + name + ":"))
    occ = int(re.search(r"; Occupancy: (\d+)", isa[end:end + 4000]).group(1))
    return {"vgpr": get("num_vgpr"), "agpr": get("num_agpr"), "scratch": get("private_seg_size"), "occupancy": occ}


@pytest.mark.parametrize("seg,twin,slots", TWINS)
def test_segmented_walk_has_no_spill_and_the_twin_occupancy(isa, seg, twin, slots):
    body = _body(isa, seg)
    merges = _walk(body)
    assert len(merges) == slots, len(merges)
    inside = [k for k in _scratch(body) if merges[0] <= k <= merges[-1]]
    assert not inside, "spill code between the merges of a step: " + "; ".join(body[k].strip() for k in inside[:5])
    # the prefetch stays in flight under the merges: no wait for the VMEM counter after it (the base address comes by scalar loads)
    dma = [k for k, l in enumerate(body) if "global_load_lds_dwordx4" in l and merges[0] <= k <= merges[-1]]
    assert dma, "the prefetch is expected between the merges of a step"
    waits = [k for k, l in enumerate(body) if "vmcnt" in l and dma[0] < k <= merges[-1]]
    assert not waits, "; ".join(body[k].strip() for k in waits[:5])
    a, b = _resources(isa, seg), _resources(isa, twin)
    assert a == b, (a, b)  # registers, scratch bytes (the prologue's, as the twin's: none of it in the walk) and waves per SIMD
    # and no scratch access anywhere the twin has none
    assert len(_scratch(body)) == len(_scratch(_body(isa, twin))), (len(_scratch(body)), len(_scratch(_body(isa, twin))))


@pytest.mark.parametrize("seg,twin", CXX_TWINS)
def test_segmented_cxx_merges_have_the_twin_resources(isa, seg, twin):
    a, b = _resources(isa, seg), _resources(isa, twin)
    assert a == b, (a, b)
    assert len(_scratch(_body(isa, seg))) == len(_scratch(_body(isa, twin)))
