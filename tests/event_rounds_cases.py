"""The builder's rounds (csrc/event_build.h: build_read): a model of the round schedule in both forms, hand-made reads
that put the carrying form (SGK_BUILD_CARRY) in each of its places, and the model that says which places a read reaches.

A builder tile is 2 048 samples; its boundaries become records in LDS and a round emits one event per lane, 64 per
round.  The parent form runs ceil(records / 64) rounds per tile.  The carrying form runs the full rounds only and keeps
the records that remain (m of them, fewer than 64) in front of the next tile's; a partial round runs in the last tile of
a walk, and in a tile that ends with fewer than 64 records of which some are leftovers already (a leftover is never older
than one tile).  A tile is too dense for the builder when its records and the leftovers exceed BREC.

The reads are staircases: plateaus of 3, 4 or 6 samples, 40 raw units apart, with noise of +-2 (the DNA preset puts a
boundary on every step; the RNA preset's windows are too long for these and get plateaus of 8, 16 and 24), and constant
stretches, which have no boundary at all.  A read is a list of tiles, each (plateaus of the short, the middle, the long
kind) and constant behind them; the numbers below were searched with the oracle (`python tests/event_rounds_cases.py`) so
that every tile holds the number of boundaries its place needs, and tests/test_event_rounds_cases_cpu.py requires every
place with the oracle's boundaries."""
import numpy as np

TILE = 2048
LANES = 64
BREC = 576


# ---------------------------------------------------------------- the round schedule, both forms
def _tiles(bounds, walk0, hi, tile):
    bounds = np.asarray(bounds, dtype=np.int64)        # in order
    edges = np.searchsorted(bounds, np.arange(walk0, hi + tile, tile))
    bounds = bounds.tolist()
    for t, tb in enumerate(range(walk0, hi, tile)):
        yield tb, bounds[edges[t]:edges[t + 1]], tb + tile >= hi


def schedule_parent(bounds, hi, walk0=0, rank0=0, skip_first=False, tile=TILE):
    """-> dict(events [(rank, previous boundary, boundary)], rounds, lanes (active ones), dense): every tile runs
    ceil(records / 64) rounds over its own records; lane 0's previous boundary is the last active lane's of the round before
    (hi: the end of the walk -- the read's or the segment's; skip_first: the first record ends no event of this walk)"""
    ev, rounds, lanes, dense, rank, prev = [], 0, 0, False, rank0, 0
    skip = rank0 if skip_first else None
    for tb, recs, _ in _tiles(bounds, walk0, hi, tile):
        if len(recs) > BREC:
            dense, recs = True, []
        for k0 in range(0, len(recs), LANES):
            part = recs[k0:k0 + LANES]
            ev.extend(zip(range(rank + k0, rank + k0 + len(part)), [prev] + part[:-1], part))
            prev = part[-1]
            rounds += 1
            lanes += len(part)
        rank += len(recs)
    ev = [e for e in ev if e[0] != skip]
    return dict(events=ev, rounds=rounds, lanes=lanes, dense=dense, rank=rank, prev=prev)


def schedule_carry(bounds, hi, walk0=0, rank0=0, skip_first=False, tile=TILE):
    """the carrying form, with the record array as it is in LDS: positions are stored relative to the tile, + one tile; a
    leftover's falls below one tile (where the look-up of the lane prefix finds zeros) and must not fall below 0.
    -> the same dict + m_in (leftovers going into each tile), totals (each tile's own boundaries), partial (tiles that ran
    a partial round), dense_by_leftovers"""
    ev, rounds, lanes, dense, rank, prev = [], 0, 0, False, rank0, 0
    skip = rank0 if skip_first else None
    lds = []                                   # stored positions of the m leftovers
    m_in, totals, partial_at, by_left = [], [], [], False
    for t, (tb, recs, last) in enumerate(_tiles(bounds, walk0, hi, tile)):
        m = len(lds)
        m_in.append(m)
        totals.append(len(recs))
        if len(recs) + m > BREC:
            dense, by_left = True, by_left or len(recs) <= BREC
            lds = []
            continue
        lds = lds + [b - tb + tile for b in recs]
        assert m == 0 or (0 <= min(lds[:m]) and max(lds[:m]) < tile)
        assert m == len(lds) or (tile <= min(lds[m:]) and max(lds[m:]) < 2 * tile)
        tot = len(lds)
        pos = [tb - tile + q for q in lds]
        nfull = tot - tot % LANES
        for k0 in range(0, nfull, LANES):
            part = pos[k0:k0 + LANES]
            ev.extend(zip(range(rank + k0, rank + k0 + LANES), [prev] + part[:-1], part))
            prev = part[LANES - 1]             # the rotate: lane 63's
            rounds += 1
            lanes += LANES
        if last or (m > 0 and tot < LANES):
            part = pos[nfull:]
            if part:
                ev.extend(zip(range(rank + nfull, rank + tot), [prev] + part[:-1], part))
                prev = part[-1]
                rounds += 1
                lanes += len(part)
                partial_at.append(t)
            rank += tot
            lds = []
        else:
            rank += nfull
            lds = [q - tile for q in lds[nfull:]]
    assert not lds
    ev = [e for e in ev if e[0] != skip]
    return dict(events=ev, rounds=rounds, lanes=lanes, dense=dense, rank=rank, prev=prev, m_in=m_in, totals=totals,
                partial=partial_at, dense_by_leftovers=by_left)


def spread(counts, tile=TILE):
    """boundary positions with counts[t] boundaries in tile t, spread evenly"""
    return [t * tile + (i * tile) // c for t, c in enumerate(counts) for i in range(c)]


# ---------------------------------------------------------------- places
PLACES = ("no_leftover_goes_into_a_tile", "1_leftover_goes_into_a_tile", "63_leftovers_go_into_a_tile",
          "a_multiple_of_64_without_leftovers_in_a_tile_that_is_not_the_last", "a_tile_without_boundaries_while_leftovers_wait",
          "the_read_ends_without_leftovers", "a_read_with_fewer_than_64_events", "a_read_of_one_tile",
          "too_dense_only_with_the_leftovers", "too_dense_by_itself")
#: plateaus long enough for the RNA preset's windows are too long for a dense tile
PLACES_OF_PRESET = {0: PLACES, 1: PLACES[:8]}


def places(bounds, n, hi=None):
    """the places a read with these boundaries reaches in a walk that starts at sample 0 and ends at hi (default: the read's
    end; a first segment's: its end.  PLACES[6], [7] and [9] are a whole read's)"""
    whole = hi is None
    hi = n if whole else hi
    bounds = np.asarray(bounds, dtype=np.int64)
    bounds = bounds[bounds < hi]
    s = schedule_carry(bounds, hi)
    out = set()
    ntiles = len(s["totals"])
    for t in range(ntiles):
        m, c = s["m_in"][t], s["totals"][t]
        if t > 0 and c + m <= BREC:
            out |= {PLACES[0]} if m == 0 else {PLACES[1]} if m == 1 else {PLACES[2]} if m == 63 else set()
        if m == 0 and c > 0 and c % LANES == 0 and t + 1 < ntiles:
            out.add(PLACES[3])
        if c == 0 and m > 0:
            out.add(PLACES[4])
        if c <= BREC < c + m:
            out.add(PLACES[8])
        if c > BREC and whole:
            out.add(PLACES[9])
    if not s["dense"]:
        if len(bounds) > 0 and (ntiles - 1) not in s["partial"]:
            out.add(PLACES[5])
        if len(bounds) + 1 < LANES and ntiles > 1 and whole:
            out.add(PLACES[6])
        if ntiles == 1 and len(bounds) > 0 and whole:
            out.add(PLACES[7])
    return out


#: segments of two tiles (tests/test_gpu_event_rounds.py): a read of more samples is cut, and its first segment walks the
#: whole read's first two tiles.  A boundary within `SEAM_MARGIN` samples in front of the seam may be the next segment's
#: (its peak was pending at the seam): a place of a first segment counts only if it is reached with and without them.
SEGMENT = 2 * TILE
SEAM_MARGIN = 8
PLACES_OF_SEGMENTS = {0: PLACES[:6] + PLACES[8:9], 1: PLACES[:6]}


def places_first_segment(bounds, n):
    if n <= SEGMENT:
        return set()
    bounds = np.asarray(bounds, dtype=np.int64)
    return places(bounds, n, SEGMENT) & places(bounds[bounds < SEGMENT - SEAM_MARGIN], n, SEGMENT)


# ---------------------------------------------------------------- the reads
NOISE_SEED = 7
PLATEAUS = {0: (3, 4, 6), 1: (8, 16, 24)}     # [rna] samples of a short, a middle, a long plateau


def build(spec, rna):
    """-> int16 read of the spec {"tiles": per tile (short, middle, long plateaus) or None: nothing but the constant, "n":
    samples of the read (the last tile may be cut short)}: per tile its staircase, the constant of the last level behind it"""
    rs = np.random.RandomState(NOISE_SEED)
    parts, level = [], 0
    for tile_spec in spec["tiles"]:
        lens = []
        if tile_spec is not None:
            for c, L in zip(tile_spec, PLATEAUS[rna]):
                lens += [L] * c
        assert sum(lens) <= TILE, (tile_spec, sum(lens))
        x = []
        for L in lens:
            level ^= 1
            x.append(500 + 40 * level + rs.randint(-2, 3, size=L))
        x.append(np.full(TILE - sum(lens), 500 + 40 * level))
        parts.append(np.concatenate(x))
    return np.concatenate(parts)[:spec["n"]].astype(np.int16)


def boundaries(oracle, raw, rna):
    """the oracle's boundaries: the start of every event but the first"""
    import event_cases as E
    ev = oracle.event_raw(np.ascontiguousarray(raw, dtype=np.int16), *E.SCALE, rna)
    return np.asarray(ev.start, dtype=np.int64)[1:]


def per_tile(bounds, n):
    return [int(((bounds >= t) & (bounds < t + TILE)).sum()) for t in range(0, n, TILE)]


#: name -> (boundaries wanted per tile (None: as many as the plateaus that fit give; ("plateaus", c): as many as c
#: plateaus give), the kind of plateau, samples of the read)
WANTED = {
    0: {"plateaus_of_4": ([None] * 4, 1, 3 * TILE + 500),                # 511, 512, 512, 125: 63 leftovers, twice
        "multiples_of_64": ([128, 64, 192], 1, 3 * TILE),                # no partial round anywhere
        "one_leftover": ([65, 130, 40], 1, 2 * TILE + 700),
        "empty_tile_behind_leftovers": ([100, 0, 0, 90], 1, 3 * TILE + 900),
        "few_events": ([("plateaus", 30), ("plateaus", 12)], 1, TILE + 600),
        "one_tile": ([("plateaus", 200)], 2, 1500),
        "dense_with_leftovers": ([511, 560, ("plateaus", 100)], 0, 2 * TILE + 1000),   # 63 + 560 > BREC >= 560
        "dense": ([None], 0, 2000)},                                      # 3-sample plateaus: 682 in a tile
    1: {"plateaus_of_8": ([None] * 4, 0, 3 * TILE + 500),
        "multiples_of_64": ([128, 64, 64], 0, 3 * TILE),
        "one_leftover": ([65, ("plateaus", 100), ("plateaus", 40)], 0, 2 * TILE + 700),
        "empty_tile_behind_leftovers": ([100, 0, 0, ("plateaus", 90)], 0, 3 * TILE + 900),
        "few_events": ([("plateaus", 30), ("plateaus", 12)], 0, TILE + 600),
        "one_tile": ([("plateaus", 80)], 1, 1500)},
}


def search(oracle, rna, name):
    """plateaus per tile such that the oracle counts the wanted boundaries in every tile"""
    want, kind, n = WANTED[rna][name]
    L = PLATEAUS[rna][kind]
    mix = name == "dense_with_leftovers"
    cnt = [(TILE // L if w is None else w[1] if isinstance(w, tuple) else w) for w in want]
    want = [None if isinstance(w, tuple) else w for w in want]

    def spec_of(cnt):
        tiles = []
        for t, c in enumerate(cnt):
            if c == 0:
                tiles.append(None)
            elif mix and want[t] == 560:       # 3- and 4-sample plateaus that fill the tile
                c4 = TILE - 3 * c
                tiles.append((c - c4, c4, 0))
            else:
                tiles.append(tuple(c if k == kind else 0 for k in range(3)))
        return dict(tiles=tiles, n=n)

    for t, w in enumerate(want):               # tile by tile: a tile's plateaus do not move the boundaries in front
        if w is None or w == 0:
            continue
        for c in sorted(range(max(1, w - 4), w + 5), key=lambda c: abs(c - w)):
            cnt[t] = c
            if per_tile(boundaries(oracle, build(spec_of(cnt), rna), rna), n)[t] == w:
                break
    spec = spec_of(cnt)
    got = per_tile(boundaries(oracle, build(spec, rna), rna), n)
    if any(w is not None and g != w for w, g in zip(want, got)):
        raise RuntimeError("no spec for %s / %d: %r" % (name, rna, got))
    return spec, got


#: [rna] -> name -> the read (what search() found; behind each: the oracle's boundaries per tile)
SPECS = {
    0: {
        'plateaus_of_4': {'tiles': [(0, 512, 0), (0, 512, 0), (0, 512, 0), (0, 512, 0)], 'n': 6644},   # [511, 512, 512, 125]
        'plateaus_of_6': {'tiles': [(0, 0, 341)] * 4, 'n': 6644},
        'multiples_of_64': {'tiles': [(0, 128, 0), (0, 64, 0), (0, 192, 0)], 'n': 6144},   # [128, 64, 192]
        'one_leftover': {'tiles': [(0, 66, 0), (0, 130, 0), (0, 39, 0)], 'n': 4796},   # [65, 130, 40]
        'empty_tile_behind_leftovers': {'tiles': [(0, 100, 0), None, None, (0, 89, 0)], 'n': 7044},   # [100, 0, 0, 90]
        'few_events': {'tiles': [(0, 30, 0), (0, 12, 0)], 'n': 2648},   # [29, 12]
        'one_tile': {'tiles': [(0, 0, 200)], 'n': 1500},   # [220]
        'dense_with_leftovers': {'tiles': [(512, 0, 0), (192, 368, 0), (100, 0, 0)], 'n': 5096},   # [511, 560, 101]
        'dense': {'tiles': [(682, 0, 0)], 'n': 2000},   # [665]
    },
    1: {
        'plateaus_of_8': {'tiles': [(256, 0, 0), (256, 0, 0), (256, 0, 0), (256, 0, 0)], 'n': 6644},   # [255, 256, 256, 62]
        'multiples_of_64': {'tiles': [(128, 0, 0), (64, 0, 0), (64, 0, 0)], 'n': 6144},   # [128, 64, 64]
        'one_leftover': {'tiles': [(65, 0, 0), (100, 0, 0), (40, 0, 0)], 'n': 4796},   # [65, 101, 41]
        'empty_tile_behind_leftovers': {'tiles': [(100, 0, 0), None, None, (90, 0, 0)], 'n': 7044},   # [100, 0, 0, 90]
        'few_events': {'tiles': [(30, 0, 0), (12, 0, 0)], 'n': 2648},   # [29, 12]
        'one_tile': {'tiles': [(0, 80, 0)], 'n': 1500},   # [84]
    },
}


def reads_of(rna):
    """-> (names, reads)"""
    names = sorted(SPECS[rna])
    return names, [build(SPECS[rna][k], rna) for k in names]


def flagged(reads):
    """the same reads with a tiny-|pA| sample (raw + offset == 1) and a large one in the constant stretch at the read's end
    or, where the staircase reaches it, in its last plateaus: they fail the exactness guard (k_event_fallback)"""
    import event_cases as E
    out = []
    for x in reads:
        y = x.copy()
        y[-3], y[-2] = int(1 - E.SCALE[1]), 32000
        out.append(y)
    return out


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle.oracle import Oracle
    o = Oracle()
    for rna_ in (0, 1):
        print("    %d: {" % rna_)
        for name_ in WANTED[rna_]:
            spec_, got_ = search(o, rna_, name_)
            print("        %r: %r,   # %r" % (name_, spec_, got_))
        print("    },")
