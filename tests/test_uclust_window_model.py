"""The window rule for UClust::Run, restated in Python beside the sequential loop of uclust.cpp:57-122 — no library, no device.

UClust::Run searches every sequence, in length order, against the centroids that exist when its turn comes: a true dependence. Most
queries do not change the index, so a WINDOW of W queries can be answered together from hit lists made on the index as it stands when
the window opens (one mpcgpu_search_pairs call: the first hit of each list whose EA reaches the threshold), and committed in order:
a query's answer stands while the index has not changed since its list was made; once a query of the window has become a centroid,
every later query's list is made again on the current index and the answer stands only if the new list equals the old one, hit by hit
and in the same order — else the window is cut there and that query opens the next one. The comparison covers the whole list:
USorter::SearchSeq orders ties through a quicksort over an array whose size is the index size (usorter.cpp:107-126), so the order
among OLD centroids can move when a centroid is added that is not itself a hit.

The model: queries 0 .. n - 1 in order, a seeded EA table, a word count per (query, centroid) from a small range so that ties abound,
and a hit list = the centroids with a count above 0, by count descending, ties by a key that depends on the index size, truncated to
MAX_REJECTS (uclust.h). Checked: assignments, centroid order and kept paths (as (query, centroid) ids) of the windowed loop equal the
sequential loop's for W = 1, 2, 7, 64 and W >= n, and the seed set holds windows without a cut, windows cut by a new hit and windows cut
by a changed tie order alone."""
import random

import pytest

MAX_REJECTS = 8
SEEDS = list(range(12))


class Instance:
    def __init__(self, seed, n=90):
        rng = random.Random(seed)
        self.n = n
        self.min_ea = 0.6
        self.ea = [[rng.random() for _ in range(n)] for _ in range(n)]
        # word counts: most pairs share no word, the others one of three counts
        self.wc = [[rng.choice([0, 0, 0, 1, 2, 3]) for _ in range(n)] for _ in range(n)]
        # an easy family: a query of it is accepted by its founder
        for q in range(n):
            f = q % 11
            if rng.random() < 0.55 and f < q:
                self.ea[q][f], self.wc[q][f] = 0.95, 3

    def hits(self, q, index):
        """SearchSeq's top list for query q on the index (centroids in insertion order): ties ordered by a key of the index size"""
        size = len(index)
        cand = [c for c in index if self.wc[q][c] > 0]
        cand.sort(key=lambda c: (-self.wc[q][c], (c * 7919 + size * 104729) % 31, c))
        return cand[:MAX_REJECTS]

    def first_hit(self, q, hits):
        """uclust.cpp:44-54"""
        for c in hits:
            if self.ea[q][c] >= self.min_ea:
                return c
        return None


def sequential(inst):
    index, rep, paths = [], {}, {}
    for q in range(inst.n):
        c = inst.first_hit(q, inst.hits(q, index))
        if c is None:
            index.append(q)
            rep[q], paths[q] = q, None  # Path.clear()
        else:
            rep[q], paths[q] = c, (q, c)
    return rep, index, paths


def windowed(inst, W, stats):
    index, rep, paths = [], {}, {}
    k = 0
    while k < inst.n:
        win = list(range(k, min(k + W, inst.n)))
        lists = {q: inst.hits(q, index) for q in win}
        answers = {q: inst.first_hit(q, lists[q]) for q in win}  # one library call for the window
        stats["calls"] += 1
        stats["sent"] += sum(len(lists[q]) for q in win)
        added, done = [], len(win)
        for i, q in enumerate(win):
            if added:
                again = inst.hits(q, index)
                if again != lists[q]:
                    stats["cut_new_hit" if set(again) & set(added) else "cut_tie_order"] += 1
                    stats["resent"] += sum(len(lists[r]) for r in win[i:])
                    done = i
                    break
            c = answers[q]
            if c is None:
                index.append(q)
                added.append(q)
                rep[q], paths[q] = q, None
            else:
                rep[q], paths[q] = c, (q, c)
        if done == len(win):
            stats["uncut"] += 1
        assert done > 0  # the first query of a window always commits
        k += done
    return rep, index, paths


def new_stats():
    return {"calls": 0, "sent": 0, "resent": 0, "uncut": 0, "cut_new_hit": 0, "cut_tie_order": 0}


@pytest.mark.parametrize("W", [1, 2, 7, 64, 1000])
def test_window_rule_equals_sequential_loop(W):
    total = new_stats()
    for seed in SEEDS:
        inst = Instance(seed)
        stats = new_stats()
        assert windowed(inst, W, stats) == sequential(inst), (seed, W)
        for key in total:
            total[key] += stats[key]
        if W == 1:
            assert stats["calls"] == inst.n and stats["cut_new_hit"] == stats["cut_tie_order"] == 0
        else:
            assert stats["calls"] < inst.n, (seed, W, stats)
    if W >= 7:  # the seed set is not trivial: every kind of window occurs
        assert total["uncut"] > 0 and total["cut_new_hit"] > 0 and total["cut_tie_order"] > 0, total


def test_whole_list_comparison_is_needed():
    """a rule that only asks "does the new list hold a new centroid" gives another clustering on some instance of the seed set"""
    def windowed_weak(inst, W):
        index, rep = [], {}
        k = 0
        while k < inst.n:
            win = list(range(k, min(k + W, inst.n)))
            lists = {q: inst.hits(q, index) for q in win}
            added, done = [], len(win)
            for i, q in enumerate(win):
                if added and set(inst.hits(q, index)) & set(added):
                    done = i
                    break
                c = inst.first_hit(q, lists[q])
                if c is None:
                    index.append(q)
                    added.append(q)
                rep[q] = q if c is None else c
            k += done
        return rep, index

    differs = 0
    for seed in SEEDS:
        inst = Instance(seed)
        ref = sequential(inst)
        differs += windowed_weak(inst, 64) != (ref[0], ref[1])
    assert differs > 0
