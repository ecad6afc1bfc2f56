"""The host-side plans of a forward (lightgaussian_amd/csrc/lg_plan.h), compiled for the CPU by tests/cpu_harness: which variant of
every kernel a view gets (ForwardPlan) and how its sort key is laid out (KeyPlan).  The expectations are written out here -- from the
expressions forward_impl used before the plan existed and from the flag documentation in include/lightgaussian.h -- not obtained from
the code under test.  No GPU."""
import ctypes as C
import itertools
import struct

import common

# include/lightgaussian.h
FAST_EXP, SKIP_COLOR, NARROW_KEY, SORT_ALL_BITS, LONG_SERIAL, LONG_PARALLEL = 2, 16, 64, 128, 512, 1024
ONE, OPACITY, ALPHA, ALPHA_T = 0, 1, 2, 3
# lg_plan.h
CHAIN_NONE, CHAIN_COLOR, CHAIN_COUNT = 0, 1, 2
SCORE_NONE, SCORE_COUNT, SCORE_COUNT_OPACITY, SCORE_SLOTS = 0, 1, 2, 3
FIELDS = ("live", "count", "exact", "color", "fscore", "merge", "clear_slots", "k1_skip_color", "k1_clears_count", "long_mode",
          "long_chain", "work_list_group", "score")


def forward_plan(flags, count, policy, N, cap):
    out = (C.c_int * len(FIELDS))()
    common.plan_harness().h_forward_plan(flags, int(count), policy, N, cap, out)
    return dict(zip(FIELDS, out))


def expected_plan(count, fast, skip, serial, parallel, policy, N, cap):
    live = cap > 0 and N > 0
    # the blend kernel's template arguments <COUNT, FSCORE, EXACT, COLOR>, as the launch ladder chose them
    nocolor = count and not fast and skip           # significance-only pass: no colour, no per-pixel outputs
    fs = 0 if not count else 2 if policy == ALPHA else 3 if policy == ALPHA_T else 0
    if not count:
        template = (False, 0, not fast, True)
    elif nocolor:
        template = (True, fs, True, False)
    else:
        template = (True, fs, not fast, True)
    merge = template[1] != 0 and not template[3]    # the kernel's own MERGE: FSCORE != 0 && !COLOR
    clear_slots = bool(fs) and live and not (not fast and skip)
    k1_clears_count = count and not (count and policy >= ALPHA)     # K1's pointer was out_count (NULL in a colour forward) unless per-hit
    cnt_par = count and not fast and skip and policy in (ONE, OPACITY)
    if not count and fast and live:
        long_mode = 0 if serial else 2 if parallel else 1
    elif cnt_par and live and parallel:
        long_mode = 2
    else:
        long_mode = 0
    par_long = long_mode != 0
    long_chain = CHAIN_COUNT if par_long and cnt_par else CHAIN_COLOR if par_long else CHAIN_NONE
    work_list_group = not (nocolor and not par_long)
    if not (count and N > 0):
        score = SCORE_NONE
    elif policy in (ONE, OPACITY):
        score = SCORE_COUNT_OPACITY if policy == OPACITY else SCORE_COUNT
    else:
        score = SCORE_SLOTS
    return dict(live=live, count=template[0], fscore=template[1], exact=template[2], color=template[3], merge=merge,
                clear_slots=clear_slots, k1_skip_color=bool(skip), k1_clears_count=k1_clears_count, long_mode=long_mode,
                long_chain=long_chain, work_list_group=work_list_group, score=score)


def _cases():
    for count, fast, skip, serial, parallel in itertools.product((False, True), repeat=5):
        flags = (FAST_EXP if fast else 0) | (SKIP_COLOR if skip else 0) | (LONG_SERIAL if serial else 0) | (LONG_PARALLEL if parallel else 0)
        for policy in (ONE, OPACITY, ALPHA, ALPHA_T):
            yield count, fast, skip, serial, parallel, policy, flags


def test_every_plan_field_over_the_whole_variant_matrix():
    variants, n = set(), 0
    for count, fast, skip, serial, parallel, policy, flags in _cases():
        # live or not (cap > 0 && N > 0): 256 cases; the two other ways of not being live ride along (the score kernel looks at N alone)
        for N, cap in ((1000, 5000), (1000, 0), (0, 5000), (0, 0)):
            got = forward_plan(flags, count, policy, N, cap)
            want = expected_plan(count, fast, skip, serial, parallel, policy, N, cap)
            assert got == {k: int(v) for k, v in want.items()}, (count, hex(flags), policy, N, cap)
            variants.add((got["count"], got["fscore"], got["exact"], got["color"]))
            n += (N, cap) in ((1000, 5000), (1000, 0))
    assert n == 256
    assert len(variants) == 11      # the lg_blend_fwd instantiations
    # bits outside the six inputs do not reach the plan
    other = 1 | 4 | 32 | NARROW_KEY | SORT_ALL_BITS | 256 | 2048 | 8192
    for count, fast, skip, serial, parallel, policy, flags in _cases():
        assert forward_plan(flags | other, count, policy, 1000, 5000) == forward_plan(flags, count, policy, 1000, 5000)


def test_slots_merge_and_score_kernel_agree():
    """What the slot clear, the kernel instantiation and the score kernel must agree on (lg_score_slots reads the slots as
    {count | weight} words: a slot that was neither cleared nor written by the merge would be a stale sort key)."""
    for count, fast, skip, serial, parallel, policy, flags in _cases():
        for live in (True, False):
            p = forward_plan(flags, count, policy, 1000, 5000 if live else 0)
            per_hit = policy in (ALPHA, ALPHA_T)
            if count:
                assert bool(p["fscore"]) == per_hit and p["fscore"] in (0, policy)
                assert bool(p["merge"]) == (per_hit and not fast and skip)
                assert bool(p["merge"]) == (per_hit and not p["color"])
                assert bool(p["color"]) == (not (not fast and skip))
                if live:
                    assert bool(p["clear_slots"]) == (per_hit and not p["merge"])
                else:
                    assert not p["clear_slots"]
                assert (p["score"] == SCORE_SLOTS) == per_hit
                assert bool(p["k1_clears_count"]) == (not per_hit)
            else:
                # a colour forward ignores the policy, and SKIP_COLOR reaches only K1
                q = forward_plan(flags, False, ONE, 1000, 5000 if live else 0)
                assert p == q
                assert p["fscore"] == 0 and not p["merge"] and not p["clear_slots"] and p["color"] and p["score"] == SCORE_NONE
                assert not p["k1_clears_count"] and p["work_list_group"]
                r = forward_plan(flags ^ SKIP_COLOR, False, policy, 1000, 5000 if live else 0)
                assert {k: v for k, v in p.items() if k != "k1_skip_color"} == {k: v for k, v in r.items() if k != "k1_skip_color"}
            assert bool(p["k1_skip_color"]) == skip
            # the exact forward runs K1 and K2 before it knows its instance count: what they read does not depend on it
            if not live:
                full = forward_plan(flags, count, policy, 1000, 5000)
                assert (p["k1_skip_color"], p["k1_clears_count"]) == (full["k1_skip_color"], full["k1_clears_count"])
            # a long-tile chain runs over the par_work list the extra workgroup builds
            assert (p["long_chain"] != CHAIN_NONE) == (p["long_mode"] != 0)
            assert p["work_list_group"] or p["long_chain"] == CHAIN_NONE


KEY_FIELDS = ("tile_bits", "gid_bits", "depth_bits", "store_drop", "two_stage", "gid_mask", "stored", "tile_shift", "sort_begin", "sort_end")


def key_plan(W, H, N, max_depth, flags=0):
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    out = (C.c_uint32 * len(KEY_FIELDS))()
    common.plan_harness().h_key_plan(ntiles, N, struct.unpack("<I", struct.pack("<f", max_depth))[0], flags, out)
    return dict(zip(KEY_FIELDS, out))


def test_key_plan_on_the_cases_its_comments_name():
    # 100.0f = 0x42C80000; minus LG_DEPTH_BIAS (124 << 23 = 0x3E000000) = 0x04C80000: patterns 0 .. 0x04C80000 need 27 bits
    # 6 M at 3840 x 2160: 240 x 135 = 32400 tiles (15 bits), ids below 2^23: 15 + 27 + 23 = 65 bits, one depth bit is not stored
    k = key_plan(3840, 2160, 6_000_000, 100.0)
    assert (k["tile_bits"], k["depth_bits"], k["gid_bits"], k["store_drop"]) == (15, 27, 23, 1)
    assert (k["stored"], k["tile_shift"], k["sort_begin"], k["sort_end"], k["gid_mask"]) == (26, 49, 49, 64, (1 << 23) - 1)
    # the frozen workload: 3 M at 1920 x 1080, 120 x 68 = 8160 tiles: 13 + 27 + 22 = 62 bits
    k = key_plan(1920, 1080, 3_000_000, 100.0)
    assert (k["tile_bits"], k["depth_bits"], k["gid_bits"], k["store_drop"], k["two_stage"]) == (13, 27, 22, 0, 1)
    assert (k["stored"], k["tile_shift"], k["sort_begin"], k["sort_end"], k["gid_mask"]) == (27, 49, 49, 62, (1 << 22) - 1)
    # ... laid out as if 40 bits were available: 62 - 40
    k = key_plan(1920, 1080, 3_000_000, 100.0, NARROW_KEY)
    assert (k["tile_bits"], k["depth_bits"], k["gid_bits"], k["store_drop"]) == (13, 27, 22, 22)
    assert (k["stored"], k["tile_shift"], k["sort_begin"], k["sort_end"]) == (5, 27, 27, 40)
    # 20 M at 1080p: ids need 25 bits, 13 + 27 + 25 = 65
    k = key_plan(1920, 1080, 20_000_000, 100.0)
    assert (k["tile_bits"], k["depth_bits"], k["gid_bits"], k["store_drop"], k["sort_end"]) == (13, 27, 25, 1, 64)
    # one-stage sort: the global passes start at the first stored depth bit instead of the tile field
    k = key_plan(1920, 1080, 3_000_000, 100.0, SORT_ALL_BITS)
    assert (k["two_stage"], k["tile_shift"], k["sort_begin"], k["sort_end"], k["store_drop"]) == (0, 49, 22, 62, 0)
    # a one-tile image has no tile bits and still sorts one
    k = key_plan(16, 16, 1000, 100.0)
    assert (k["tile_bits"], k["gid_bits"], k["depth_bits"], k["store_drop"]) == (0, 10, 27, 0)
    assert (k["tile_shift"], k["sort_begin"], k["sort_end"]) == (37, 37, 38)
    # at least one depth bit is always stored: 20 M at 3840 x 2160 in 40 bits leaves none (15 + 25 = 40), 26 of the 27 are dropped
    k = key_plan(3840, 2160, 20_000_000, 100.0, NARROW_KEY)
    assert (k["tile_bits"], k["depth_bits"], k["gid_bits"], k["store_drop"], k["stored"]) == (15, 27, 25, 26, 1)
    # a depth maximum at or below the bias (an empty view reads back 0) still has a one-bit depth field; N = 0 and 1 a one-bit id
    for N in (0, 1, 2):
        k = key_plan(640, 480, N, 0.0)
        assert (k["tile_bits"], k["depth_bits"], k["gid_bits"], k["gid_mask"], k["store_drop"], k["stored"]) == (11, 1, 1, 1, 0, 1)
    # very wide fields (2^30 tiles, 2^29 - 1 Gaussians, +inf = 0x7F800000): 30 + 31 + 29 = 90 bits, 26 dropped
    k = key_plan(16 * 32768, 16 * 32768, (1 << 29) - 1, float("inf"))
    assert (k["tile_bits"], k["depth_bits"], k["gid_bits"], k["store_drop"], k["stored"], k["sort_end"]) == (30, 31, 29, 26, 5, 64)
