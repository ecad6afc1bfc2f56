/* lightgaussian_blocks.h -- extension of the C ABI of liblightgaussian_hip.so (include/lightgaussian.h and lightgaussian_mesh.h, same ABI
 * version): a block-sparse TSDF volume for unbounded scenes.  It fuses the depth maps lg_tsdf_integrate takes into blocks allocated from
 * those maps and extracts the same marching-tetrahedra mesh across block borders.  Error codes, lg_last_error(), LG_FLAG_PROFILE and the
 * stream argument are lightgaussian.h's; views are lightgaussian_mesh.h's lg_tsdf_view.  DESIGN.md section 10.15 holds the contract and
 * its reasons; lightgaussian_amd/csrc/lg_math.h writes every operation out in order.
 *
 * --- the volume: lg_block_volume ----------------------------------------------------------------------------------------------------
 * An unbounded lattice: point (i, j, k) lies at origin + voxel_size (i, j, k), evaluated per axis as the dense volume evaluates it.  A
 * block is 8 x 8 x 8 points, block coordinate b = floor(i / 8) in [-2^20, 2^20) per axis, key = (bz + 2^20) << 42 | (by + 2^20) << 21 |
 * (bx + 2^20).  keys [n_blocks] (int64) is strictly ascending and storage follows it, x fastest inside a block: tsdf [n,8,8,8] (fresh
 * value 1), weight [n,8,8,8] (fresh value 0), color [n,8,8,8,3] or NULL (fresh value 0).  n_blocks 512 < 2^29; 0 < trunc <= 4 voxel_size.
 * tsdf, weight and color are 16-byte aligned, keys 8-byte.
 *
 * --- lg_blocks_touch / lg_blocks_merge: which blocks the views need -------------------------------------------------------------------
 * lg_blocks_touch runs one lane per pixel.  A pixel takes part when its depth d is positive and finite, not above a positive depth_max,
 * and its alpha, when given, not below alpha_min.  With r = (((2 ix + 1) / W - 1) tanfovx, ((2 iy + 1) / H - 1) tanfovy, 1), a_w and b_w
 * the world points of r (d - trunc) and r (d + trunc) under the view matrix taken as rigid, and pad = voxel_size + (d + trunc)
 * sqrt((tanfovx / W)^2 + (tanfovy / H)^2), the pixel touches every block of the lattice box [min(a_w, b_w) - pad, max(a_w, b_w) + pad].
 * It is skipped and counted when the box spans more than 4 blocks along an axis or a lattice index leaves [-2^23, 2^23).  Equal keys are
 * removed inside each wave of 8 x 8 pixels; what is left goes to candidates [capacity] (int64), the rest of which is filled with -1.
 * stats (DEVICE int64[4]) receives [1] = the number of candidates the views produced and [2] = the skipped pixels; when [1] > capacity the
 * candidates are incomplete and the caller repeats the call with a larger buffer.  scratch: lg_blocks_touch_scratch_bytes(n_views, views).
 * One call takes views of fewer than 2^26 pixels in all.
 * lg_blocks_merge writes the sorted union of old_keys [n_old] and the non-negative keys of add_keys [n_add] to merged (room for n_old +
 * n_add) and their number to count (DEVICE int64; -1 when the radix sort gave up and the list is void): the new key list.  The set is the contract; it does not depend on the order of
 * add_keys or on capacity.  scratch: lg_blocks_merge_scratch_bytes(n_old + n_add).  n_old + n_add < 2^30.
 *
 * --- lg_blocks_regrid: a new pool from the old one ----------------------------------------------------------------------------------
 * Every element of `to` is written with plain stores: a block whose key exists in `from` keeps its 512 values bit for bit, any other
 * block gets the fresh values.  Both volumes keep colour or neither does.
 *
 * --- lg_blocks_integrate ------------------------------------------------------------------------------------------------------------
 * lg_tsdf_integrate's per-point text at every point of every block, with the global lattice index; views in order, 8 per launch; one
 * call with n views gives the bits of n calls with one view.  A block behind a view's z_min plane is skipped whole for that view.
 *
 * --- lg_blocks_mesh_count / lg_blocks_mesh_emit ---------------------------------------------------------------------------------------
 * lg_mesh_count / lg_mesh_emit's rules over the lattice: the point at p + offset(m) may live in one of the seven + neighbour blocks; a
 * missing block is unobserved.  Vertex ids count the carrying edges by (block rank, point in block, slot), faces are ordered by (block
 * rank, cell in block, tetrahedron, triangle); a cell belongs to the block of its corner 0.  Vertex position = origin + voxel_size
 * ((float)global index + t offset).  The count / read counts / allocate / emit protocol, the refusal of counts that differ from those in
 * scratch and the scratch alignment (256) are lg_mesh_emit's; scratch: lg_blocks_mesh_scratch_bytes(n_blocks).
 * flags: LG_FLAG_PROFILE records "blocks_touch" (lg_blocks_touch and lg_blocks_merge, once per call), "blocks_regrid",
 * "blocks_integrate" (per launch), "blocks_mesh_count", "blocks_mesh_scan", "blocks_mesh_emit".
 * LG_ERR_INVALID_ARGUMENT, before any device call, the message naming the argument: a null pointer (color, view color / alpha and colors
 * excepted; keys, tsdf and weight of a volume without blocks too) or a misaligned one; n_blocks < 0 or n_blocks 512 >= 2^29; voxel_size not
 * positive and finite; trunc outside (0, 4 voxel_size]; a non-finite origin or iso; min_weight not positive and finite; a NaN tanfovx /
 * tanfovy, z_min, depth_max or alpha_min; W or H outside [1, 32768]; negative counts or capacities; a view without color for a volume
 * that keeps colour; colors for a volume that keeps none. */
#ifndef LIGHTGAUSSIAN_BLOCKS_H
#define LIGHTGAUSSIAN_BLOCKS_H

#include "lightgaussian_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lg_block_volume {
    float origin[3];
    float voxel_size;
    float trunc;
    int32_t n_blocks;
    const int64_t* keys;
    float* tsdf;
    float* weight;
    float* color;
} lg_block_volume;

size_t lg_blocks_touch_scratch_bytes(int32_t n_views, const lg_tsdf_view* views);
int lg_blocks_touch(const lg_block_volume* volume, int32_t n_views, const lg_tsdf_view* views, int64_t capacity, int64_t* candidates, int64_t* stats,
                    void* scratch, uint32_t flags, void* stream);
size_t lg_blocks_merge_scratch_bytes(int64_t n);
int lg_blocks_merge(int64_t n_old, const int64_t* old_keys, int64_t n_add, const int64_t* add_keys, int64_t* merged, int64_t* count, void* scratch,
                    uint32_t flags, void* stream);
int lg_blocks_regrid(const lg_block_volume* from, const lg_block_volume* to, uint32_t flags, void* stream);
int lg_blocks_integrate(const lg_block_volume* volume, int32_t n_views, const lg_tsdf_view* views, uint32_t flags, void* stream);
size_t lg_blocks_mesh_scratch_bytes(int32_t n_blocks);
int lg_blocks_mesh_count(const lg_block_volume* volume, float iso, float min_weight, void* scratch, int64_t* counts, uint32_t flags, void* stream);
int lg_blocks_mesh_emit(const lg_block_volume* volume, float iso, float min_weight, void* scratch, int64_t n_vertices, int64_t n_faces, float* vertices,
                        float* colors, int32_t* faces, uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIGHTGAUSSIAN_BLOCKS_H */
