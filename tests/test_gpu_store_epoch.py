"""mpcgpu_store_epoch on the device (include/mpcgpu.h): the counter a caller keeps beside the fingerprint of what a store was
computed from. Readers leave it, everything that replaces or invalidates tables, sequences, pair order, shard, store or
committed values moves it, a refused call leaves it — and an unmoved epoch means the store still gives the oracle's join
(tests/_store_epoch.py; 8 x 60 family)."""
import pytest

import _store_epoch as SE

pytestmark = pytest.mark.gpu


def test_readers_leave_the_epoch():
    SE.check_readers_leave_it()


@pytest.mark.parametrize("name", sorted(SE.MOVERS))
def test_epoch_moves(name):
    SE.check_mover(name)


def test_list_stage_moves_the_epoch():
    SE.check_list_stage_moves_it()


def test_new_context_is_zero_and_refused_calls_leave_it():
    SE.check_new_context_and_refusals()


def test_epoch_guards_a_reused_store():
    SE.check_epoch_guards_reuse()


def test_group_calls_move_every_context():
    SE.check_group_moves_every_context(devices=(0, 0))
