"""fb_chain_mega_kernel on the device: chain sweeps of structure-profile (.mega) input, MPCGPU_FB_CHAIN_MEGA (0 never, 1 wherever the
kernel launches, 2 the rule; unset: never). Every case compares EA bits, nnz, offsets, columns and value bits of all pairs with two
references: the oracle (or the bb11001 golden) and the same stage under MPCGPU_FB_CHAIN=0. Every environment setting runs in a
child process of its own under a time limit (tests/_mega_chains.py); a run that several tests need is made once.

Small lists are cut into chains of one by the grading of build_chains (the short end of a launch: fewer pairs than resident waves),
so the cases that count chains run with MPCGPU_FB_CHAIN_GRADE=0, as the byte suites do."""
import numpy as np
import pytest

import _golden as G
import _mega_chains as MC
import _parity as P

pytestmark = pytest.mark.gpu

ON0 = dict(MC.ON, **MC.GRADE0)


def _pairs(n):
    return n * (n - 1) // 2


def test_bb11001_chains_against_golden():
    """83, 85, 91, 86 residues, two rows per lane: (0,1) (0,2) (0,3) and (1,2) (1,3) chain. On the code before fb_chain_mega_kernel a
    .mega run reports no chained pair (and has no stage_a_chain_bins)."""
    m = G.mega("mega_bb11001")
    off = MC.child("bb11001", MC.OFF)[0]
    for tag, env in (("MPCGPU_FB_CHAIN_MEGA=1", ON0), ("unset", {}), ("MPCGPU_FB_CHAIN_MEGA=1, graded", MC.ON)):
        got = MC.child("bb11001", env)[0]
        MC.same(tag, got, m["ea"], m["stage"][0])
        assert G.stage_digest(got["store"]) == m["digest"][0], tag
        MC.same(tag + " against MPCGPU_FB_CHAIN=0", got, off["ea"], off["store"])
    on = MC.child("bb11001", ON0)[0]
    assert on["info"][1] > 0 and on["info"][2] > 0, on["info"]
    assert on["info"] == (6, 5, 2) and on["bins"] == [2], (on["info"], on["bins"])
    assert off["info"] == (6, 0, 0) and off["bins"] == [], (off["info"], off["bins"])


@pytest.mark.parametrize("nfeat", [1, 3, 8])
def test_synthetic_profiles_against_oracle(nfeat):
    """20 sequences in the bins of 1 .. 4 rows per lane, ragged alphabets, 1, 3 and MPC_MEGA_FMAX features; LY + 1 == T chains,
    LY + 1 < T leaves the chain (MC.SYNTH)"""
    name = "synth_f%d" % nfeat
    want, want_ea = MC.oracle(name)
    on, off = MC.child(name, ON0)[0], MC.child(name, MC.OFF)[0]
    MC.same("MPCGPU_FB_CHAIN_MEGA=1", on, want_ea, want)
    MC.same("MPCGPU_FB_CHAIN=0", off, want_ea, want)
    MC.same("against MPCGPU_FB_CHAIN=0", on, off["ea"], off["store"])
    exp = MC.expected_chains(MC.SYNTH)
    assert on["info"] == (_pairs(20),) + exp, (on["info"], exp)
    assert on["bins"] == [1, 2, 3, 4], on["bins"]
    assert off["info"] == (_pairs(20), 0, 0) and off["bins"] == []
    # T - 1 and T - 2 residues behind the row sequences of 250 and 126 (T = 63): restated, so that the lengths keep meaning it
    assert MC.lanes_t(250) == MC.lanes_t(126) == 63 and 62 in MC.SYNTH[2:] and 61 in MC.SYNTH[2:]


@pytest.mark.parametrize("cmax", [2, 3])
def test_chain_length_limit(cmax):
    want, want_ea = MC.oracle("synth_f8")
    on = MC.child("synth_f8", dict(ON0, MPCGPU_FB_CHAIN_MAX=str(cmax)))[0]
    off = MC.child("synth_f8", MC.OFF)[0]
    MC.same("MPCGPU_FB_CHAIN_MAX=%d" % cmax, on, want_ea, want)
    MC.same("against MPCGPU_FB_CHAIN=0", on, off["ea"], off["store"])
    assert on["info"] == (_pairs(20),) + MC.expected_chains(MC.SYNTH, cmax), on["info"]


def test_chain_of_sixteen_and_two():
    """19 sequences, the default limit of 16: the first row sequence has 18 partners, one chain of 16 and one of 2"""
    want, want_ea = MC.oracle("n19_f8")
    on, off = MC.child("n19_f8", ON0)[0], MC.child("n19_f8", MC.OFF)[0]
    MC.same("MPCGPU_FB_CHAIN_MEGA=1", on, want_ea, want)
    MC.same("against MPCGPU_FB_CHAIN=0", on, off["ea"], off["store"])
    exp = MC.expected_chains(MC.N19)
    assert MC.expected_chains(MC.N19[:1] + MC.N19[1:])[0] >= 18 and MC.lanes_t(MC.N19[0]) <= min(MC.N19[1:]) + 1
    assert on["info"] == (_pairs(19),) + exp, (on["info"], exp)


def test_graded_chains():
    """grading on (the default): the short end of a launch is cut into shorter chains; whatever the cut, the same results"""
    want, want_ea = MC.oracle("synth_f8")
    on, off = MC.child("synth_f8", MC.ON)[0], MC.child("synth_f8", MC.OFF)[0]
    MC.same("graded", on, want_ea, want)
    MC.same("graded against MPCGPU_FB_CHAIN=0", on, off["ea"], off["store"])
    assert on["bins"] == [1, 2, 3, 4] and on["info"][0] == _pairs(20), (on["bins"], on["info"])


def test_pair_list_with_profiles_chains():
    """mpcgpu_align_msas on 12 pairs, eight of them in a row with one seq1, profiles loaded: path, score and EA bits against the
    restatement of test_align_msas_vs_restatement (with the profiles' emissions), and chains formed"""
    path, sc, ea = MC.msas_restatement("synth_f8")
    on = MC.child("msas:synth_f8", ON0)[0]
    off = MC.child("msas:synth_f8", MC.OFF)[0]
    for tag, got in (("MPCGPU_FB_CHAIN_MEGA=1", on), ("MPCGPU_FB_CHAIN=0", off)):
        assert got["path"] == path and P.bits(got["score"]) == P.bits(sc), tag
        assert np.array_equal(P.bits(got["ea"]), P.bits(ea)), tag
    assert on["info"] == (12,) + MC.MSAS_CHAINED and on["bins"] == [2], (on["info"], on["bins"])
    assert off["info"] == (12, 0, 0) and off["bins"] == []


def test_row_block_pairs_stay_out_of_the_chains():
    """a row sequence of 800 residues between short ones: its four pairs take the row-block kernel (or the cooperative one), the 11
    others one chain launch of two rows per lane. Launch counters and trace lines state the split."""
    want, want_ea = MC.oracle("rowblock_f8")
    trace = {"MPCGPU_TRACE": "1"}
    on, lines = MC.child("rowblock_f8", dict(ON0, **trace))
    off, lines0 = MC.child("rowblock_f8", dict(MC.OFF, **trace))
    MC.same("MPCGPU_FB_CHAIN_MEGA=1", on, want_ea, want)
    MC.same("MPCGPU_FB_CHAIN=0", off, want_ea, want)
    assert on["info"] == (15,) + MC.expected_chains(MC.ROWBLOCK) == (15, 10, 3), on["info"]
    assert on["bins"] == [2] and off["bins"] == []
    assert on["fb_launches"] == 2 and off["fb_launches"] == 2, (on["fb_launches"], off["fb_launches"])  # row blocks + one bin
    assert MC.trace_bins(lines, "[mpcgpu] fb row blocks: H=") == {7: 4} == MC.trace_bins(lines0, "[mpcgpu] fb row blocks: H=")
    assert MC.trace_bins(lines, "[mpcgpu] fb chain members H=") == {2: 11} and not MC.trace_bins(lines, "[mpcgpu] fb H=")
    assert MC.trace_bins(lines0, "[mpcgpu] fb H=") == {2: 11} and not MC.trace_bins(lines0, "[mpcgpu] fb chain members H=")


def test_letters_after_a_chained_mega_stage():
    """mpcgpu_set_mega(nfeat = 0) after a chained .mega stage: the byte stage on the same context equals a fresh context's"""
    want, want_ea = MC.oracle("synth_f3")
    got = MC.child("letters:synth_f3", ON0)[0]
    MC.same("the .mega stage", got, want_ea, want)
    assert got["info"][1] > 0
    MC.same("letters after .mega", got["letters"], got["fresh"]["ea"], got["fresh"]["store"])
    assert got["letters"]["info"] == got["fresh"]["info"] and got["letters"]["bins"] == got["fresh"]["bins"]
    assert not np.array_equal(P.bits(got["ea"]), P.bits(got["letters"]["ea"]))


@pytest.mark.parametrize("knob", [None, "2"])
def test_rule_bins_are_the_bins_that_chain(knob):
    """the rule (2) and the unset knob: the trace names `fb chains H=` for every bin of stage_a_chain_bins() and for no other, and
    the results are those of MPCGPU_FB_CHAIN=0. Which bins the rule takes is the chip's to say (registers and residency of each
    instantiation); unset takes none."""
    env = dict(MC.GRADE0, MPCGPU_TRACE="1")
    if knob is not None:
        env["MPCGPU_FB_CHAIN_MEGA"] = knob
    got, lines = MC.child("synth_f3", env)
    off = MC.child("synth_f3", MC.OFF)[0]
    want, want_ea = MC.oracle("synth_f3")
    MC.same("knob %s" % knob, got, want_ea, want)
    MC.same("knob %s against MPCGPU_FB_CHAIN=0" % knob, got, off["ea"], off["store"])
    named = sorted({int(ln.split("H=", 1)[1].split()[0]) for ln in lines if ln.startswith("[mpcgpu] fb chains H=")})
    assert named == got["bins"], (named, got["bins"])
    assert set(got["bins"]) <= {1, 2, 3, 4}
    singles = MC.trace_bins(lines, "[mpcgpu] fb H=")
    members = MC.trace_bins(lines, "[mpcgpu] fb chain members H=")
    assert sum(singles.values()) + sum(members.values()) == _pairs(20), (singles, members)
    if knob is None:
        assert got["bins"] == [] and got["info"][1:] == (0, 0), (got["bins"], got["info"])
