"""The rule behind the chaining stage's lazy primary (fg_chain.hip lazy_primary), checked against a plain
Python restatement of the reference's backtracking and primary selection (overlap.cpp:331-439) on random DP tables.

The DP leaves element 0 with score 0 and no back pointer, every other element without one (a root) with score exactly
k, every element with one (live) with score > k, and back[i] < i.  The rule: let e* be the live element of the
STRICTLY largest score (1); if its chain is rooted at element 0 or no element points at element 0 (2), and the
candidate of its whole chain passes overlapTest (3), that candidate is the only_max_ext primary -- under every order
std::sort may leave tied scores in, for the chain starts and for the candidates alike.
"""
import random

K = 17


def select_primary(score, back, test, start_ties, cand_ties, k=K):
    """overlap.cpp:331-439 with only_max_ext: chain starts by descending score, walks that consume the back pointers,
    ``test(first, last)`` for overlapTest, candidates by descending score, front().  ``*_ties``: how a sort leaves
    elements of equal score: "stable", "reversed", or a random.Random that shuffles them."""
    def ordered(items, key, ties):
        items = list(items)
        if ties == "reversed":
            items.reverse()
        elif ties != "stable":
            ties.shuffle(items)
        return sorted(items, key=key)          # Python's sort is stable: ties stay as arranged above

    back = list(back)
    cands = []
    for start in ordered(range(len(score)), lambda i: -score[i], start_ties):
        if back[start] == -1:
            continue
        pos, first, length = start, 0, 0
        while pos != -1:
            first = pos
            length += 1
            nxt = back[pos]
            back[pos] = -1
            pos = nxt
        if test(first, start):
            cands.append((first, start, length, score[start] - score[first] + k - 1))
    cands = ordered(cands, lambda c: -c[3], cand_ties)
    return cands[0] if cands else None


def lazy_rule(score, back, test, k=K, use=(True, True, True)):
    """("fast", candidate), ("none", None) for a group without a live element, or ("full", reason).  ``use`` switches
    the three conditions off one by one (to show that each is needed)."""
    live = [i for i in range(len(score)) if back[i] != -1]
    if not live:
        return "none", None
    top = max(score[i] for i in live)
    holders = [i for i in live if score[i] == top]
    if use[0] and len(holders) > 1:
        return "full", "tied_top"
    last = holders[0]
    first, length, pos = last, 0, last
    while pos != -1:
        first = pos
        length += 1
        pos = back[pos]
    if use[1] and first != 0 and any(b == 0 for b in back):
        return "full", "root"
    if use[2] and not test(first, last):
        return "full", "overlap_test"
    return "fast", (first, last, length, score[last] - score[first] + k - 1)


def random_table(rng, n, p_root, narrow, k=K):
    """A forest with back[i] < i and scores that keep the DP's invariants.  ``narrow``: live scores from a few values
    just above k (many ties, scores unrelated to the chains) instead of rising along the chain."""
    score, back = [0], [-1]
    for i in range(1, n):
        if rng.random() < p_root:
            back.append(-1)
            score.append(k)
        else:
            b = rng.randrange(0, i) if rng.random() < 0.5 else max(0, i - 1 - rng.randrange(0, 3))
            back.append(b)
            score.append(k + 1 + rng.randrange(0, 6) if narrow else max(score[b], k) + 1 + rng.randrange(0, k))
    return score, back


def check_invariants(score, back, k=K):
    assert score[0] == 0 and back[0] == -1
    for i in range(1, len(score)):
        assert -1 <= back[i] < i
        assert score[i] == k if back[i] == -1 else score[i] > k


TIE_ORDERS = ["stable", "reversed"]


def all_selections(score, back, test, seed=0):
    out = [select_primary(score, back, test, a, b) for a in TIE_ORDERS for b in TIE_ORDERS]
    r = random.Random(seed)
    out += [select_primary(score, back, test, r, r) for _ in range(3)]
    return out


def test_rule_agrees_with_the_full_selection_on_random_tables():
    rng = random.Random(20241)
    outcomes = {"fast": 0, "none": 0, "tied_top": 0, "root": 0, "overlap_test": 0}
    many_cands = planted = rooted0 = rooted_elsewhere = 0
    for it in range(6000):
        n = rng.choice([1, 2, 3, 5, 8, 13, 30, 70, 150])
        score, back = random_table(rng, n, rng.choice([0.05, 0.3, 0.6, 1.0]), narrow=rng.random() < 0.4)
        if rng.random() < 0.3 and n > 3:       # no element points at element 0: chains rooted elsewhere only
            for i in range(1, n):
                if back[i] == 0:
                    back[i], score[i] = -1, K
        if rng.random() < 0.2:                  # a planted tie: some live element gets the score of another
            live = [i for i in range(n) if back[i] != -1]
            if len(live) >= 2:
                a, b = rng.sample(live, 2)
                score[a] = score[b]
                planted += 1
        check_invariants(score, back)
        salt, mod = rng.randrange(1000), rng.choice([1, 2, 3, 7])
        test = (lambda f, l: True) if mod == 1 else (lambda f, l, s=salt, m=mod: (f * 31 + l * 17 + s) % m != 0)
        verdict, cand = lazy_rule(score, back, test)
        sel = all_selections(score, back, test, it)
        if verdict == "fast":
            assert all(s == cand for s in sel), (score, back, cand, sel)
            rooted0 += cand[0] == 0
            rooted_elsewhere += cand[0] != 0
        elif verdict == "none":
            assert all(s is None for s in sel)
        outcomes[cand if verdict == "full" else verdict] += 1
        # how many candidates the full path had (cases above std::sort's 16-element insertion sort threshold)
        b2, nc = list(back), 0
        for s in sorted(range(n), key=lambda i: -score[i]):
            if b2[s] != -1:
                nc += 1
                p = s
                while p != -1:
                    nxt = b2[p]
                    b2[p] = -1
                    p = nxt
        many_cands += nc > 16 and verdict == "fast"
    assert all(v > 50 for v in outcomes.values()), outcomes
    assert many_cands > 20 and planted > 200 and rooted0 > 100 and rooted_elsewhere > 100


def test_a_tied_top_score_needs_the_full_path():
    # two chains whose ends share the top score: the start order decides which candidate comes first
    score = [0, K, 30, K, 30]
    back = [-1, -1, 1, -1, 3]
    check_invariants(score, back)
    ok = lambda f, l: True
    assert lazy_rule(score, back, ok) == ("full", "tied_top")
    _, naive = lazy_rule(score, back, ok, use=(False, True, True))
    assert select_primary(score, back, ok, "stable", "stable") == naive == (1, 2, 2, 29)
    assert select_primary(score, back, ok, "reversed", "stable") == (3, 4, 2, 29) != naive


def test_a_chain_rooted_at_element_zero_can_outscore_the_top_element():
    # element 0 has score 0, every other root k: a short chain rooted there gains k on the best chain
    score = [0, 25, K, 30]
    back = [-1, 0, -1, 2]
    check_invariants(score, back)
    ok = lambda f, l: True
    assert lazy_rule(score, back, ok) == ("full", "root")
    _, naive = lazy_rule(score, back, ok, use=(True, False, True))
    assert naive == (2, 3, 2, 29)
    assert set(all_selections(score, back, ok)) == {(0, 1, 2, 41)}
    # the same table with the best chain rooted at element 0 is fast
    back2 = [-1, 0, -1, 1]
    assert lazy_rule(score, back2, ok) == ("fast", (0, 3, 3, 46))
    assert set(all_selections(score, back2, ok)) == {(0, 3, 3, 46)}


def test_a_best_chain_that_fails_overlap_test_needs_the_full_path():
    score = [0, K, 40, K, 30]
    back = [-1, -1, 1, -1, 3]
    check_invariants(score, back)
    test = lambda f, l: l != 2
    assert lazy_rule(score, back, test) == ("full", "overlap_test")
    _, naive = lazy_rule(score, back, test, use=(True, True, False))
    assert naive == (1, 2, 2, 39)
    assert set(all_selections(score, back, test)) == {(3, 4, 2, 29)}


def test_a_lower_start_on_the_best_chain_is_cut_at_the_consumed_node():
    # the walk from 4 stops at 2, which the best chain (5 -> 2 -> 1) has consumed: its candidate scores
    # score[4] - score[2] + k - 1, below the bound the rule's proof uses
    score = [0, K, 28, K, 35, 50]
    back = [-1, -1, 1, -1, 2, 2]
    check_invariants(score, back)
    ok = lambda f, l: True
    assert lazy_rule(score, back, ok) == ("fast", (1, 5, 3, 49))
    assert set(all_selections(score, back, ok)) == {(1, 5, 3, 49)}
