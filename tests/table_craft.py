"""The k-mer lookup table of fg_index.hip (fgIndexLookupStructures, k_table_insert) and fg_ctx.h (fg_probe), restated in
plain Python, and crafted indexes whose keys are chosen by their home group (tests only, no device).

The table: narrow form (k <= 17) one 64-bit slot ``key << 30 | index inside the part`` (index bits all ones: a
repetitive k-mer), wide form (k >= 18) ``{key, index}`` pairs.  A part has ``groups`` 8-slot groups.  An insert walks
slot by slot from the key's start slot (narrow: the first slot of its home group; wide: ``home * 8 + (mix & 7)``) to
the first empty one, wrapping from the part's end to its start.  A narrow probe reads whole groups from the home group
and stops at the first one that holds the key or has an empty slot; a wide probe reads slots from the start slot and
stops at the key or at an empty slot.  More than FG_TABLE_PART_KEYS keys are cut into key-range parts of that many kept
keys; repetitive k-mers go into the part their value falls in.

What of this does not depend on the order of insertion (the device inserts concurrently) is stated as such: the set
of occupied slots of a part, hence the whole walk of an absent k-mer, and the bounds `stored_beyond` gives by counting.
Where a statement needs a placement (the walk of one present key), the restatement uses two insertion orders and the
device tests read the real placement through fg_debug_table."""
from __future__ import annotations

import numpy as np

import chain_craft as cc

U64 = np.uint64
EMPTY = 0xFFFFFFFFFFFFFFFF
IDX_BITS = 30
IDX_MASK = (1 << IDX_BITS) - 1
MAX_PARTS = 16
DEFAULT_PART_KEYS = (1 << IDX_BITS) - 2
MIN_GROUPS = 16
MIN_OVERLAP = cc.MIN_OVERLAP


# ---- hashing ---------------------------------------------------------------------------------------------------------
def fg_mix(x):
    """the 64-bit finalizer of fg_ctx.h on an array of keys (arithmetic modulo 2^64)"""
    x = np.array(x, dtype=U64, ndmin=1, copy=True)
    with np.errstate(over="ignore"):
        x ^= x >> U64(33)
        x *= U64(0xff51afd7ed558ccd)
        x ^= x >> U64(33)
        x *= U64(0xc4ceb9fe1a85ec53)
        x ^= x >> U64(33)
    return x


def home_group(keys, n_groups):
    """umulhi(mix >> 32, n_groups)"""
    return (((fg_mix(keys) >> U64(32)) * U64(n_groups)) >> U64(32)).astype(np.int64)


def wide_start(keys, n_groups):
    """the wide form's start slot, home * 8 + (mix & 7)"""
    return home_group(keys, n_groups) * 8 + (fg_mix(keys) & U64(7)).astype(np.int64)


def start_slot(keys, n_groups, wide):
    return wide_start(keys, n_groups) if wide else home_group(keys, n_groups) * 8


def part_of(keys, bound):
    """part p holds the keys in [bound[p], bound[p + 1]); bound has n_parts + 1 entries, the last is never compared"""
    keys = np.array(keys, dtype=U64, ndmin=1)
    inner = np.asarray(bound, U64)[1:-1]
    return np.searchsorted(inner, keys, side="right").astype(np.int64)


# ---- geometry --------------------------------------------------------------------------------------------------------
def is_wide(k):
    return 2 * k > 64 - IDX_BITS


def load_pct(n_keep, n_rep, env_pct=None):
    """FG_TABLE_LOAD_PCT clamped to 5..90; without it 25 while the table stays small, else 50"""
    if env_pct is not None:
        return max(5, min(90, int(env_pct)))
    return 25 if (n_keep + n_rep) * 32 <= (2 << 30) else 50


def groups_for(n, pct):
    return max(MIN_GROUPS, (n * 100 // pct + 7) // 8)


class Geometry:
    """parts, key_base, kept keys and stored candidates (kept + repetitive) per part, groups, slot_base; ``bound`` where
    the key values are known"""

    def __init__(self, wide, key_base, kept, part_keys, groups, slot_base, bound=None):
        self.wide, self.n_parts = bool(wide), len(groups)
        self.key_base, self.kept, self.part_keys = list(key_base), list(kept), list(part_keys)
        self.groups, self.slot_base = list(groups), list(slot_base)
        self.n_slots = sum(groups) * 8
        self.bound = None if bound is None else [int(b) for b in bound]

    def same_shape(self, other):
        return (self.wide == other.wide and self.key_base == other.key_base and self.kept == other.kept and
                self.part_keys == other.part_keys and self.groups == other.groups and self.slot_base == other.slot_base)

    def __repr__(self):
        return (f"Geometry(wide={self.wide}, parts={self.n_parts}, key_base={self.key_base}, part_keys={self.part_keys}, "
                f"groups={self.groups}, slot_base={self.slot_base})")


def n_parts_for(n_keep, k, part_keys_env=None):
    per = DEFAULT_PART_KEYS if part_keys_env is None else int(part_keys_env)
    return 1 if is_wide(k) or n_keep == 0 else (n_keep + per - 1) // per


def geometry(n_keep, n_rep, k, part_keys_env=None, load_pct_env=None):
    """The table's shape from the counts alone: ``n_rep`` = repetitive keys per part (a list, or their number where
    there is one part).  n_keep counts every key of the sorted key array, those with an empty list included."""
    wide = is_wide(k)
    per = DEFAULT_PART_KEYS if part_keys_env is None else int(part_keys_env)
    n_parts = n_parts_for(n_keep, k, part_keys_env)
    assert n_parts <= MAX_PARTS
    rep = [int(n_rep)] if np.isscalar(n_rep) else [int(r) for r in n_rep]
    assert len(rep) == n_parts, "one count of repetitive keys per part"
    pct = load_pct(n_keep, sum(rep), load_pct_env)
    key_base = [0 if wide else p * per for p in range(n_parts)]
    kept = [min(n_keep - key_base[p], n_keep if wide else per) for p in range(n_parts)]
    part_keys = [kept[p] + rep[p] for p in range(n_parts)]
    groups = [groups_for(n, pct) for n in part_keys]
    slot_base = [8 * sum(groups[:p]) for p in range(n_parts)]
    return Geometry(wide, key_base, kept, part_keys, groups, slot_base)


def geometry_of(keys, rep, k, part_keys_env=None, load_pct_env=None):
    """The table's shape for a finished key set: the bounds are the first key of each part"""
    keys, rep = np.asarray(keys, U64), np.asarray(rep, U64)
    n_parts = n_parts_for(len(keys), k, part_keys_env)
    per = DEFAULT_PART_KEYS if part_keys_env is None else int(part_keys_env)
    bound = [0] + [int(keys[p * per]) for p in range(1, n_parts)] + [EMPTY]
    rp = np.bincount(part_of(rep, bound), minlength=n_parts) if len(rep) else np.zeros(n_parts, np.int64)
    g = geometry(len(keys), [int(x) for x in rp], k, part_keys_env, load_pct_env)
    g.bound = bound
    return g


# ---- insertion and walks ---------------------------------------------------------------------------------------------
def insert(start, n_slots, order):
    """linear probing from ``start[j]`` in the order given: slot -> j, -1 where empty"""
    slots = -np.ones(n_slots, np.int64)
    for j in order:
        h = int(start[j])
        while slots[h] >= 0:
            h = 0 if h + 1 == n_slots else h + 1
        slots[h] = j
    return slots


def stored_keys(ex):
    """(key, index in the key array or -1 for a repetitive key) of everything the table stores: keys with a non-empty
    list and the repetitive keys"""
    cnt = np.diff(ex.key_off.astype(np.int64))
    idx = np.nonzero(cnt > 0)[0]
    keys = np.concatenate([ex.keys[idx], np.asarray(ex.repetitive, U64)])
    return keys.astype(U64), np.concatenate([idx, -np.ones(len(ex.repetitive), np.int64)])


class PartTable:
    """One part after insertion: ``occ`` the occupied slots (the same for every insertion order, asserted on two),
    ``place`` the slot -> stored-key placement of ascending key order, ``keys`` the part's stored keys"""

    def __init__(self, keys, n_groups, wide, start=None):
        self.keys, self.n_groups, self.wide = keys, n_groups, wide
        self.n = n_groups * 8
        if start is None:           # (tests of this class give the start slots themselves)
            start = start_slot(keys, n_groups, wide) if len(keys) else np.zeros(0, np.int64)
        self.start = np.asarray(start, np.int64)
        fwd = insert(self.start, self.n, range(len(keys)))
        rev = insert(self.start, self.n, range(len(keys) - 1, -1, -1))
        assert np.array_equal(fwd >= 0, rev >= 0), "the occupied slot set depends on the insertion order"
        self.place, self.place_rev = fwd, rev
        self.occ = fwd >= 0
        assert int(self.occ.sum()) == len(keys) < self.n
        # per start unit (narrow: group, wide: slot): units a miss reads, and whether it passes the part's end
        if wide:
            free = ~self.occ
        else:
            free = ~self.occ.reshape(n_groups, 8).all(axis=1)
        m = len(free)
        nxt = np.zeros(m, np.int64)        # distance to the first unit with an empty slot, in units
        d = None
        for i in list(range(m - 1, -1, -1)) * 2:
            d = 0 if free[i] else (d + 1 if d is not None else None)
            if d is not None:
                nxt[i] = d
        self.miss_len = nxt + 1
        self.miss_wraps = np.arange(m) + nxt >= m

    def unit(self, slot):
        return slot if self.wide else slot // 8

    def walk_to(self, start, slot):
        """(units read, wrapped) of the probe of a key that starts at slot ``start`` and is stored at ``slot``; asserts
        that nothing on the way lets the probe stop early"""
        u0, u1, m = self.unit(int(start)), self.unit(int(slot)), self.n if self.wide else self.n_groups
        n = (u1 - u0) % m + 1
        assert n <= self.miss_len[u0], "an empty slot lies before the key on its own walk"
        return n, u0 + n - 1 >= m


def build_parts(ex, geom):
    """PartTable of every part of the index's table"""
    keys, _ = stored_keys(ex)
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    part = part_of(keys, geom.bound)
    return [PartTable(keys[part == p], geom.groups[p], geom.wide) for p in range(geom.n_parts)]


def stored_beyond(pt, first_unit, n_units, homes_in):
    """At least this many stored keys whose start lies in the ``homes_in`` units from ``first_unit`` sit outside the
    ``n_units`` units from ``first_unit`` in EVERY insertion order -- provided no key starts in the rest of that
    window: the window's slots cannot hold them all.  (Units: groups; a wide part counts start slots by their group.)"""
    g = pt.start // 8
    rel = (g - first_unit) % pt.n_groups
    assert not np.any((rel >= homes_in) & (rel < n_units)), "a key starts in the window's tail"
    return max(0, int((rel < homes_in).sum()) - 8 * n_units)


# ---- reads -----------------------------------------------------------------------------------------------------------
def canonical(seq, k):
    fw, rv = cc.kmer_codes(seq, k)
    return np.minimum(fw, rv), rv < fw


class Reads:
    """A few dozen random reads of 2-3 kb and reads cut with overlaps from one random sequence (every second one stored
    reverse-complemented), so that overlap records exist"""

    def __init__(self, seed, n_random=48, genome_len=9000, read_len=3000, step=750):
        rng = np.random.default_rng(seed)
        self.seqs, self.from_genome = [], []
        genome = rng.integers(0, 4, size=genome_len, dtype=np.uint8)
        self.genome = genome
        for i, a in enumerate(range(0, genome_len - read_len + 1, step)):
            s = genome[a:a + read_len]
            self.seqs.append(np.ascontiguousarray(cc.revcomp(s) if i & 1 else s))
            self.from_genome.append(True)
        for _ in range(n_random):
            self.seqs.append(rng.integers(0, 4, size=int(rng.integers(2000, 3001)), dtype=np.uint8))
            self.from_genome.append(False)

    def readset(self):
        from flye_amd import synth
        return synth.ReadSet.from_arrays(self.seqs)

    def candidates(self, k):
        """(distinct canonical k-mers of all reads ascending, True where the k-mer lies in the overlapping reads)"""
        allk = np.unique(np.concatenate([canonical(s, k)[0] for s in self.seqs]))
        gen = np.unique(np.concatenate([canonical(s, k)[0] for s, g in zip(self.seqs, self.from_genome) if g]))
        return allk, np.isin(allk, gen)

    def shared_kmers(self, k):
        """canonical k-mers of the stretch every cut read but the outermost ones shares with its neighbours"""
        return np.unique(canonical(self.genome[3000:len(self.genome) - 3000], k)[0])

    def index(self, k, keys, repetitive=(), empty=()):
        """IndexExport in fg_export_index's layout: ``keys`` (and the ``empty`` ones, listed without entries) ascending,
        each kept key with ALL its occurrences at positions 0 .. len-k-1 of every read, record = 2 * read + strand of
        the canonical form, position on that strand, ascending per key.  Repetitive keys get no list."""
        from oracle import oracle as O
        keys = np.unique(np.asarray(keys, U64))
        empty = np.unique(np.asarray(empty, U64))
        rep = np.unique(np.asarray(repetitive, U64))
        assert not np.intersect1d(keys, rep).size and not np.intersect1d(keys, empty).size
        assert not np.intersect1d(empty, rep).size
        kk, ee = [np.empty(0, U64)], [np.empty(0, U64)]
        for r, s in enumerate(self.seqs):
            can, flip = canonical(s, k)
            pos = np.nonzero(np.isin(can, keys))[0]
            f = flip[pos]
            rec = 2 * r + f.astype(np.int64)
            p = np.where(f, len(s) - pos - k, pos)
            kk.append(can[pos])
            ee.append((rec.astype(U64) << U64(32)) | p.astype(U64))
        kk, ee = np.concatenate(kk), np.concatenate(ee)
        order = np.lexsort((ee, kk))
        kk, ee = kk[order], ee[order]
        assert np.array_equal(np.unique(kk), keys), "a key of the case occurs nowhere"
        allkeys = np.union1d(keys, empty)
        off = np.zeros(len(allkeys) + 1, U64)
        off[1:] = np.searchsorted(kk, allkeys, side="right").astype(U64)
        return O.IndexExport(np.ascontiguousarray(allkeys), off, np.ascontiguousarray(ee), np.ascontiguousarray(rep))


_READS = {}


def reads_for(seed=20240):
    if seed not in _READS:
        _READS[seed] = Reads(seed)
    return _READS[seed]


# ---- cases -----------------------------------------------------------------------------------------------------------
class Picker:
    """Takes candidate k-mers by predicate, those of the overlapping reads first, never one twice"""

    def __init__(self, cand, from_genome, seed):
        self.cand, self.gen = cand, from_genome
        self.free = np.ones(len(cand), bool)
        self.rng = np.random.default_rng(seed)

    def take(self, mask, n, genome_share=1.0, what=""):
        """n candidates with ``mask``; at most ceil(n * genome_share) of them from the overlapping reads"""
        m = mask & self.free
        g, o = np.nonzero(m & self.gen)[0], np.nonzero(m & ~self.gen)[0]
        ng = min(len(g), int(np.ceil(n * genome_share)))
        if n - ng > len(o):
            ng = n - len(o)
        assert 0 <= ng <= len(g) and n - ng <= len(o), f"not enough candidates {what}: {n} of {len(g)} + {len(o)}"
        pick = np.concatenate([self.rng.choice(g, ng, replace=False), self.rng.choice(o, n - ng, replace=False)])
        self.free[pick] = False
        return self.cand[pick.astype(np.int64)]


class TableCase:
    """A crafted index with the environment its table is built under and what it planned"""

    def __init__(self, name, k, reads, ex, env, plan, notes=None):
        self.name, self.k, self.reads, self.ex, self.env, self.plan = name, k, reads, ex, dict(env), plan
        self.notes = notes or {}
        self.geom = geometry_of(ex.keys, ex.repetitive, k, env.get("FG_TABLE_PART_KEYS"), env.get("FG_TABLE_LOAD_PCT"))
        if plan is not None:
            assert self.geom.same_shape(plan), f"{name}: planned {plan}, the finished key set gives {self.geom}"
        self._parts = None

    def with_env(self, **env):
        e = dict(self.env)
        e.update(env)
        return TableCase(self.name, self.k, self.reads, self.ex, e, None, self.notes)

    @property
    def parts(self):
        if self._parts is None:
            self._parts = build_parts(self.ex, self.geom)
        return self._parts

    def readset(self):
        return self.reads.readset()

    def queries(self):
        return np.arange(0, 2 * len(self.reads.seqs), dtype=np.uint32)

    def probed(self):
        """every distinct canonical k-mer the queries probe, with its class: 0 absent, 1 present (non-empty list),
        2 repetitive, 3 key with an empty list"""
        cand, _ = self.reads.candidates(self.k)
        cls = np.zeros(len(cand), np.int64)
        cnt = np.diff(self.ex.key_off.astype(np.int64))
        cls[np.isin(cand, self.ex.keys[cnt > 0])] = 1
        cls[np.isin(cand, self.ex.repetitive)] = 2
        cls[np.isin(cand, self.ex.keys[cnt == 0])] = 3
        return cand, cls

    def walks(self, placement=None):
        """Per probed k-mer: (class, part, units read, wrapped).  Absent k-mers and keys with an empty list walk to the
        first unit with an empty slot; a stored key walks to where ``placement`` (per part: slot -> index into the
        part's keys; default: ascending insertion) has it."""
        cand, cls = self.probed()
        g = self.geom
        part = part_of(cand, g.bound)
        units, wraps = np.zeros(len(cand), np.int64), np.zeros(len(cand), bool)
        for p, pt in enumerate(self.parts):
            sel = np.nonzero(part == p)[0]
            st = start_slot(cand[sel], pt.n_groups, g.wide)
            u0 = st if g.wide else st // 8
            units[sel], wraps[sel] = pt.miss_len[u0], pt.miss_wraps[u0]
            if not len(pt.keys):
                continue
            place = pt.place if placement is None else placement[p]
            where = np.zeros(len(pt.keys), np.int64)
            where[place[place >= 0]] = np.nonzero(place >= 0)[0]
            at = np.minimum(np.searchsorted(pt.keys, cand[sel]), len(pt.keys) - 1)
            for i in np.nonzero(pt.keys[at] == cand[sel])[0]:
                units[sel[i]], wraps[sel[i]] = pt.walk_to(st[i], where[at[i]])
        return cand, cls, part, units, wraps

    def stats(self, placement=None):
        """walk statistics over the probed k-mers, by class"""
        cand, cls, part, units, wraps = self.walks(placement)
        names = {0: "absent", 1: "present", 2: "repetitive", 3: "empty_list"}
        out = dict(probed=len(cand), multi=int((units > 1).sum()), wrapped=int(wraps.sum()),
                   inside_part=len(cand), max_units=int(units.max()) if len(units) else 0)
        for c, nm in names.items():
            m = cls == c
            out[nm] = int(m.sum())
            out[nm + "_multi"] = int((units[m] > 1).sum())
            out[nm + "_wrapped"] = int(wraps[m].sum())
            out[nm + "_max"] = int(units[m].max()) if m.any() else 0
        return out


CLUSTER = (19, 12, 12, 0, 0)            # keys per home group g, g + 1, ...: 43 keys that 40 slots cannot hold
N_CHAIN = 115                           # at FG_TABLE_LOAD_PCT=90: (115 * 100 / 90 + 7) / 8 = 16 groups, 128 slots


def chain_case(k, wrap=False, seed=1):
    """115 stored keys in 16 groups.  19 share home group g, 12 each have g + 1 and g + 2, none g + 3 or g + 4: whatever
    the insertion order, at least 3 of the 43 sit in group g + 5 or later (three groups or more from home), and at
    least 11 of the 19 outside g.  The other 11 home groups get 6 or 7 keys each.  Two keys are repetitive: one of
    the 19, and one of home g + 1 that lies in the stretch the cut reads share.  wrap: g is the last group."""
    reads = reads_for()
    cand, gen = reads.candidates(k)
    env = {"FG_TABLE_LOAD_PCT": "90"}
    n_rep = 2
    plan = geometry(N_CHAIN - n_rep, n_rep, k, None, 90)
    G = plan.groups[0]
    assert G == 16 and plan.n_slots == 128
    g = G - 1 if wrap else 5
    home = home_group(cand, G)
    pk = Picker(cand, gen, seed + 100 * k + (7 if wrap else 0))
    shared = np.isin(cand, reads.shared_kmers(k))
    counts = {(g + i) % G: c for i, c in enumerate(CLUSTER)}
    rest = [x for x in range(G) if x not in counts]
    spare = N_CHAIN - sum(CLUSTER)
    for i, x in enumerate(rest):
        counts[x] = spare // len(rest) + (1 if i < spare % len(rest) else 0)
    rep = [pk.take((home == g) & gen, 1, what="rep g")[0], pk.take((home == (g + 1) % G) & shared, 1, what="rep g+1")[0]]
    keys = []
    for x, c in counts.items():
        c -= (x == g) + (x == (g + 1) % G)
        if c:
            keys.append(pk.take(home == x, c, what=f"home {x}"))
    keys = np.concatenate(keys)
    assert len(keys) + len(rep) == N_CHAIN
    ex = reads.index(k, keys, rep)
    return TableCase("wrap" if wrap else "chain", k, reads, ex, env, plan,
                     dict(g=g, rep_in_cluster=int(rep[0]), rep_in_overlap=int(rep[1])))


PART_KEYS = 497
N_PARTS_KEEP = 4 * PART_KEYS + 1        # 5 parts, the last with one kept key
N_LAST = 10                             # ... and 9 repetitive keys above it: 10 keys of home 15 in a 16-group part


def parts_case(k, seed=3):
    """2000 stored keys (1989 kept + 11 repetitive) with FG_TABLE_PART_KEYS=497: parts 0-3 hold 497 kept keys in 249
    groups, part 4 one kept key and 9 repetitive ones above it in the 16-group minimum.  Every part has 12 (part 4: all
    10) keys whose home is its last group: at least 4 (2) of them wrap to the part's own group 0 in every order.
    Repetitive keys: one below bound[1] (home: the last group of part 0), one between part 1's last kept key and
    bound[2], nine at or above the last bound.  The bounds are kept keys with lists, so they are probed."""
    assert not is_wide(k)
    reads = reads_for()
    cand, gen = reads.candidates(k)
    env = {"FG_TABLE_PART_KEYS": str(PART_KEYS)}
    plan = geometry(N_PARTS_KEEP, [1, 1, 0, 0, N_LAST - 1], k, PART_KEYS, None)
    assert plan.groups == [249, 249, 249, 249, 16] and plan.n_parts == 5
    pk = Picker(cand, gen, seed + 100 * k)
    N = len(cand)
    idx = np.arange(N)
    # the last part: the top of the value range, 10 keys of home 15 (of 16); the smallest is the kept one = bound[4]
    top = 0
    while True:
        top += 200
        m = (idx >= N - top) & (home_group(cand, 16) == 15)
        if m.sum() >= N_LAST:
            break
    last = np.sort(cand[np.nonzero(m)[0][-N_LAST:]])
    pk.free[np.isin(cand, last)] = False
    lo_last = np.nonzero(cand == last[0])[0][0]
    keys, rep = [last[:1]], [last[1:]]
    cuts = [lo_last * p // 4 for p in range(5)]
    for p in range(4):
        inr = (idx >= cuts[p]) & (idx < cuts[p + 1])
        G = plan.groups[p]
        home = home_group(cand, G)
        body = inr & (idx < cuts[p + 1] - 50)       # the range's top 50 stay free for a key between the parts
        if p == 0:
            rep.append(pk.take(body & (home == G - 1), 1, what="rep part 0"))
        if p == 1:
            rep.append(pk.take(inr & ~body, 1, what="rep between"))
        keys.append(pk.take(body & (home == G - 1), 12, genome_share=0.5, what=f"last group of part {p}"))
        keys.append(pk.take(body & (home != G - 1), PART_KEYS - 12, genome_share=0.6, what=f"part {p}"))
    keys, rep = np.concatenate(keys), np.concatenate(rep)
    ex = reads.index(k, keys, rep)
    c = TableCase("parts", k, reads, ex, env, plan)
    b = c.geom.bound
    srt = np.sort(keys)
    c.notes = dict(rep_below_bound1=int((rep < b[1]).sum()), rep_at_or_above_last=int((rep >= b[4]).sum()),
                   rep_between=int(((rep > srt[2 * PART_KEYS - 1]) & (rep < b[2])).sum()))
    return c


def degenerate_case(k, which, seed=5):
    """(a) repetitive keys only, (b) one key, (c) keys with empty lists among normal ones"""
    reads = reads_for()
    cand, gen = reads.candidates(k)
    pk = Picker(cand, gen, seed + 100 * k)
    shared = np.isin(cand, reads.shared_kmers(k))
    if which == "a":
        ex = reads.index(k, [], pk.take(shared, 24))
        plan = geometry(0, 24, k)
    elif which == "b":
        ex = reads.index(k, pk.take(shared, 1))
        plan = geometry(1, 0, k)
    else:
        ex = reads.index(k, pk.take(shared, 300), pk.take(shared, 5), pk.take(shared, 40))
        plan = geometry(340, 5, k)
    return TableCase("degenerate_" + which, k, reads, ex, {}, plan)


def make_case(name, k):
    if name == "chain":
        return chain_case(k)
    if name == "wrap":
        return chain_case(k, wrap=True)
    if name == "parts":
        return parts_case(k)
    if name.startswith("degenerate_"):
        return degenerate_case(k, name[-1])
    raise KeyError(name)


_CASES = {}


def get_case(name, k):
    """cases are built once per process and never changed"""
    if (name, k) not in _CASES:
        _CASES[(name, k)] = make_case(name, k)
    return _CASES[(name, k)]
