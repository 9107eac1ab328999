"""post_ea_kernel on the device: the case table of tests/_ea.py — mpcgpu_ea_scores at 0 ulp against the CPU oracle's EA and against
mpcgpu_calc_posteriors + mpcgpu_get_ea on a second context, the route of every case by mpcgpu_ea_info and the launch counters, a call
beside a store, refusals by name."""
import pytest
import torch  # before the library is loaded: one HIP runtime in the process, the one the CU count is read from

import _ea

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", _ea.CASES)
def test_ea_case(name):
    if name in _ea.CASES_DEVICE:  # the persistent loop iterates on THIS device: the batch is larger than any grid the launcher can give it
        c = _ea.case(name)
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        smem, _ = _ea.post_ea_smem(_ea.lens_of(c), c["env"])
        B = len(_ea.pairs_of(c))
        print(name, "CUs", cus, "smem", smem, "pairs", B, "grid at the most", _ea.grid_bound(c, cus))
        assert B > cus * (_ea.POST_EA_LDS_PER_CU // smem), (name, "too many CUs for this list: every workgroup would finish one pair", cus, smem, B)
    _ea.check_case(name)


def test_ea_inert_beside_a_store():
    _ea.check_inert()


def test_ea_refusals():
    _ea.check_refusals()
