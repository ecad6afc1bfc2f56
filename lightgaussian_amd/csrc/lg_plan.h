// lg_plan.h -- host-side plans of one forward: KeyPlan (layout of the sort key) and ForwardPlan (which variant of every kernel the view gets).
// Plain C++17 on top of the public header: no HIP, no kernel header -- tests/cpu_harness compiles it with g++ and tests/test_forward_plan.py
// pins every field.  lg_api.hip reads these plans and decides nothing about variants on its own.
#pragma once
#include <stdint.h>
#include <algorithm>
#include "../../include/lightgaussian.h"
#include "../../include/lightgaussian_score.h"   // LG_FLAG_SCORE_MAX

static inline int bits_for(uint32_t n) // smallest b with 2^b >= n
{
    int b = 0;
    while (b < 32 && (1ull << b) < n) b++;
    return b;
}
// the Gaussian-id field of the sort keys / list entries: a function of N alone, so the backward and the lg_debug_* readers find the forward's
static inline int lg_gid_bits(int N) { return bits_for((uint32_t)(N > 1 ? N : 2)); }
static inline uint32_t lg_gid_mask(int gid_bits) { return gid_bits >= 32 ? 0xFFFFFFFFu : ((1u << gid_bits) - 1u); }

// Layout of the sort key of one view: tile | (depth bits - bias) >> store_drop | Gaussian id.  Exact forward: from the
// read-back depth maximum.  Bounded forward: from the caller's depth bound (nothing is read back).
#define LG_DEPTH_BIAS (124u << 23) // bit pattern of 0.125f < the 0.2 near plane
#define LG_NARROW_KEY_BITS 40   // LG_FLAG_NARROW_KEY (cross-check): lay the key out as if only this many bits were available
struct KeyPlan {
    int tile_bits, gid_bits, depth_bits;   // field widths; depth_bits = width of the FULL depth pattern (minus bias) of this view
    int store_drop;                        // low depth bits that are not stored in the key (the fields exceed 64 bits): 0 at C3
    bool two_stage;                        // radix passes on the tile bits only + lg_tile_sort (default); false = LG_FLAG_SORT_ALL_BITS
    uint32_t gid_mask;
    int stored() const { return depth_bits - store_drop; }
    int tile_shift() const { return gid_bits + stored(); }
    // bit span of the global radix passes: the tile field (at least one bit: a single-tile image still needs its keys moved to the
    // output buffer), preceded by every stored depth bit in the one-stage scheme
    int sort_begin() const { return two_stage ? tile_shift() : gid_bits; }
    int sort_end() const { return tile_shift() + (tile_bits > 0 ? tile_bits : 1); }
    int sort_passes() const { return (sort_end() - sort_begin() + 7) / 8; }   // 8-bit digits
};
static inline KeyPlan make_key_plan(int ntiles, int N, uint32_t dmax_bits, uint32_t flags)
{
    KeyPlan k;
    k.tile_bits = bits_for((uint32_t)ntiles);
    k.gid_bits = lg_gid_bits(N);
    const uint32_t dspan = dmax_bits > LG_DEPTH_BIAS ? dmax_bits - LG_DEPTH_BIAS : 0u;
    k.depth_bits = bits_for(dspan + 1u) > 0 ? bits_for(dspan + 1u) : 1;
    // The three fields must fit 64 bits.  When they do not (6 M Gaussians at 3840x2160: 15 + 27 + 23 = 65; 20 M at 1080p; ...)
    // the lowest depth bits are left out of the key and the tile sort reads the full depth pattern from the binning record
    // (tinfo) -- r2 fell back to a (tile << 32 | depth, id) pair sort through hipCUB there, without the bounded
    // forward, the graph and the fused histograms.  At least one depth bit is always stored (tile <= 32 bits, id <= 29).
    const int avail = (flags & LG_FLAG_NARROW_KEY) ? LG_NARROW_KEY_BITS : 64;
    k.store_drop = std::max(0, std::min(k.depth_bits - 1, k.tile_bits + k.depth_bits + k.gid_bits - avail));
    // Two-stage sort (default, round 3): the global radix passes cover the tile bits only (13 bits at 1080p: two 8-bit passes
    // instead of the four that tile + 19 depth bits took in round 2) and lg_tile_sort orders every list on ALL depth bits inside
    // LDS.  LG_FLAG_SORT_ALL_BITS keeps the one-stage scheme -- every stored bit through the global passes, lg_tile_ranges
    // finishing the bits a key beyond 64 bits does not store -- as an independent cross-check.
    k.two_stage = !(flags & LG_FLAG_SORT_ALL_BITS);
    k.gid_mask = lg_gid_mask(k.gid_bits);
    return k;
}

// Which variant of every kernel one forward launches.  Made by make_forward_plan before the launches that read it; every fact is
// computed here once and read by name everywhere else.
enum { LG_CHAIN_NONE = 0, LG_CHAIN_COLOR = 1, LG_CHAIN_COUNT = 2 };                                     // ForwardPlan::long_chain
enum { LG_SCORE_NONE = 0, LG_SCORE_COUNT = 1, LG_SCORE_COUNT_OPACITY = 2, LG_SCORE_SLOTS = 3, LG_SCORE_SLOTS_MAX = 4 };   // ForwardPlan::score
// The one definition of "this lg_blend_fwd<COUNT, FSCORE, EXACT, COLOR> merges its per-hit words in LDS and stores every slot once": the kernel's
// MERGE and ForwardPlan::merge (hence clear_slots) both come from here.  A variant that adds into its slots with atomics needs them cleared first;
// were the two to disagree, lg_score_slots would read stale sort keys as {count | weight} words.
constexpr bool lg_blend_merges(int fscore, bool color) { return fscore != 0 && !color; }
struct ForwardPlan {
    // lg_blend_fwd<count, fscore, exact, color, fmax>: 15 of the 48 combinations exist (colour forward: exact or not; count forward with an
    // image: 3 policies x exact or not; significance-only: 3 policies; LG_FLAG_SCORE_MAX: the 2 per-hit policies, canonical exp, with or without the image)
    bool live;               // the view has Gaussians and instances (cap > 0 && N > 0): without them the blend kernel still runs (background, zero
                             // counts) but there is nothing to bin, clear or walk in parallel
    bool count;              // count forward: hit counts and scores are wanted (a colour forward ignores the weight policy)
    bool exact;              // canonical exp (bit-pinned); false = hardware exp / rcp, LG_FLAG_FAST_EXP
    bool color;              // false = significance-only pass: no colour, no per-pixel outputs (count forward, canonical exp, LG_FLAG_SKIP_COLOR)
    int fscore;              // per-hit weights: 0, or LG_WEIGHT_ALPHA / LG_WEIGHT_ALPHA_T (= the kernels' LG_W_ALPHA / LG_W_ALPHA_T) -- the kernel is
                             // instantiated per policy and adds {count | Q8.40 weight} words into the instances' pre-sort slots: the radix sort's
                             // input buffer (keys_in), free since lg_tile_sort
    bool fmax;               // LG_FLAG_SCORE_MAX on a per-hit policy: the slot words are {count : 16 at bit 48 | fp32 bits of the largest weight : 32 low} and
                             // lg_score_slots<true> takes the maximum over a Gaussian's slots.  Everything else of the plan is the sum's: same slots, same
                             // merge / clear rule, same serial walk
    bool merge;              // per-hit weights of the significance-only pass: the waves of a tile merge in LDS and write every slot exactly once
    bool clear_slots;        // ... every other per-hit variant adds into its slots with atomics, and the slots are cleared before the blend
    bool k1_skip_color;      // LG_FLAG_SKIP_COLOR as K1 sees it (count forward or not): no SH rows read, no dynamic-LDS pad
    bool k1_clears_count;    // K1 clears the count / score accumulators for the integer weights; the per-hit policies accumulate in the slots and
                             // lg_score_slots writes both outputs
    int long_mode;           // long per-tile lists: 0 = every list is walked serially inside lg_blend_fwd, 1 = "auto" (which lists go through the
                             // parallel kernels is decided ON THE DEVICE from this view's own instance count, lg_par_min), 2 = every multi-segment list
    int long_chain;          // the kernels behind lg_blend_fwd when long_mode != 0: lg_blend_fwd_seg / _rewalk (colour) or lg_count_seg / _rewalk / _fixup
    bool work_list_group;    // lg_blend_fwd's grid has one workgroup past the tiles: it builds the backward's work list from the tile ranges, and the
                             // par_work list the long-tile chain runs over (the significance-only pass has no backward: only with a chain)
    int score;               // the kernel that closes a count view: lg_score_kernel (unit or opacity weights) over the counts, or lg_score_slots
};
// cap: instances the binning buffer holds -- R itself (exact forward) or the caller's capacity (bounded)
static inline ForwardPlan make_forward_plan(uint32_t flags, bool count, int weight_policy, int N, int64_t cap)
{
    const bool fast = flags & LG_FLAG_FAST_EXP;
    const bool want_serial = flags & LG_FLAG_LONG_SERIAL, want_parallel = flags & LG_FLAG_LONG_PARALLEL;
    ForwardPlan p;
    p.live = cap > 0 && N > 0;
    p.count = count;
    p.exact = !fast;
    p.k1_skip_color = flags & LG_FLAG_SKIP_COLOR;
    p.color = !(count && p.exact && p.k1_skip_color);
    p.fscore = (count && (weight_policy == LG_WEIGHT_ALPHA || weight_policy == LG_WEIGHT_ALPHA_T)) ? weight_policy : 0;
    p.fmax = p.fscore && (flags & LG_FLAG_SCORE_MAX);
    p.merge = lg_blend_merges(p.fscore, p.color);
    p.clear_slots = p.fscore && !p.merge && p.live;
    p.k1_clears_count = count && !p.fscore;
    // Long tiles of the hardware-exp colour forward: no history, no host hint -- two renders of the same inputs run the same kernels on
    // the same lists whatever the process rendered before.  LG_FLAG_LONG_SERIAL / _PARALLEL override the default rule per call; the
    // canonical / count variants always walk serially (bit-pinned).
    // Round 5: the significance-only pass with integer weights has a parallel long-tile walk of its own (lg_count_seg / _rewalk / _fixup:
    // bit-identical counts through interval comparisons + an exact fix-up); count forwards that return an image and the float weight
    // policies walk serially.
    // The default rule ("auto") applies to the colour forward only.  For the significance pass it was measured and lost (heavy-tailed scene,
    // four views in flight as prune_list_sharded runs them: 1150 views/s against 1497 serial): the serial walk of a pile stops
    // early in every wave whose pixels saturate, the parallel one walks every segment twice, and with other views in flight the device is
    // never idle behind the one long walk -- total work decides, not the critical path.  LG_FLAG_LONG_PARALLEL selects it explicitly.
    p.long_mode = 0;
    p.long_chain = LG_CHAIN_NONE;
    if (p.live && !count && fast) {
        p.long_mode = want_serial ? 0 : want_parallel ? 2 : 1;
        if (p.long_mode) p.long_chain = LG_CHAIN_COLOR;
    } else if (p.live && !p.color && !p.fscore && want_parallel) {
        p.long_mode = 2;
        p.long_chain = LG_CHAIN_COUNT;
    }
    p.work_list_group = p.color || p.long_chain != LG_CHAIN_NONE;
    p.score = !(count && N > 0) ? LG_SCORE_NONE : p.fscore ? (p.fmax ? LG_SCORE_SLOTS_MAX : LG_SCORE_SLOTS) : weight_policy == LG_WEIGHT_OPACITY ? LG_SCORE_COUNT_OPACITY : LG_SCORE_COUNT;
    return p;
}
