"""All-pairs stage A (mpcgpu_calc_posteriors) on MI355X at production shapes, every path of its dispatcher and batch pipeline pinned bit
for bit against the oracle: every rows-per-lane instantiation of the three forward/backward families at both edges of its class, the
row-block threshold and instantiations, both finishing kernels by their own conditions, one / many / single-pair batches, a pair
sub-range, candidate-overflow retries alone and inside a run of batches, the growing shard buffer, one context reused. Each run
proves its path by launch counters (in this process, batches overlapping as in production) and by MPCGPU_TRACE lines (in a child
process under its own timeout; nothing is retried); tests/_stage_a.py holds the table and the path map."""
import pytest

import _stage_a as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_stage_a_case(name):
    S.run_case(S.case("gpu", name), "gpu")
    S.check_case_traced("gpu", name)
