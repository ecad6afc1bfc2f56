// CPU harness around the PRODUCT's host-side plans (lightgaussian_amd/csrc/lg_plan.h): the key layout and the kernel-variant
// decisions of a forward, field by field, for tests/test_forward_plan.py.  Test infrastructure, compiled with g++; no GPU.
#include "../../lightgaussian_amd/csrc/lg_plan.h"

extern "C" {

void h_key_plan(int ntiles, int N, uint32_t dmax_bits, uint32_t flags, uint32_t* out10)
{
    const KeyPlan k = make_key_plan(ntiles, N, dmax_bits, flags);
    const uint32_t f[10] = { (uint32_t)k.tile_bits, (uint32_t)k.gid_bits, (uint32_t)k.depth_bits, (uint32_t)k.store_drop, k.two_stage, k.gid_mask,
                             (uint32_t)k.stored(), (uint32_t)k.tile_shift(), (uint32_t)k.sort_begin(), (uint32_t)k.sort_end() };
    for (int i = 0; i < 10; i++) out10[i] = f[i];
}

void h_forward_plan(uint32_t flags, int count, int weight_policy, int N, long long cap, int* out13)
{
    const ForwardPlan p = make_forward_plan(flags, count != 0, weight_policy, N, cap);
    const int f[13] = { p.live, p.count, p.exact, p.color, p.fscore, p.merge, p.clear_slots, p.k1_skip_color, p.k1_clears_count,
                        p.long_mode, p.long_chain, p.work_list_group, p.score };
    for (int i = 0; i < 13; i++) out13[i] = f[i];
}
}
