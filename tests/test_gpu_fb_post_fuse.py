"""fb_chain_post_kernel on the device: a wave that has swept a chain finishes the chain's pairs before it takes the next one
(MPCGPU_FB_POST_FUSE). Cases and comparisons: tests/_fb_post_fuse.py."""
import pytest

import _fb_post_fuse as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", F.NAMES)
def test_fused_finish_matches_separate_launch_and_oracle(name):
    F.check(name)


def test_default_rule():
    F.check_default()
