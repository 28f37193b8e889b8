// edge_core.h -- the deblocking edge bits of one 4x4 luma unit from the CU / TU structure (derive_edgeFlags, deblock.cc:31-237;
// the host helper de265hip_derive_edge_flags restates it CB by CB).  Here the work is split by UNIT instead of by CB: a lane finds
// the CB that covers its unit, walks that CB's transform tree down to the leaf that holds the unit, and knows the unit's whole
// edge byte.  No lane writes anything but its own unit's byte, so the body runs as a plain grid on the device (k_scan.hip:
// workgroups of k_scan_tus, or k_edge_flags) and as a loop on the host (dry builds, the CPU tests), compiled from this file.
#pragma once
#include "dev_common.h"

namespace d265 {

#define EDGE_FN __host__ __device__ inline

// what the body reads, in a structured picture's arena (uploaded with it; the pointers are the arena's device addresses)
struct EdgeJob {
  const uint8_t* cb_log2;              // per MinCb unit, cbs_w x cbs_h: log2 CB size at a CB's top-left unit, 0 elsewhere
  const uint8_t* cb_part;              // per MinCb unit: PartMode at the top-left unit
  const uint8_t* tu_split;             // per MinTb unit over whole CTBs, tbs_w wide: bit d = split_transform_flag at depth d
  const de265hip_ctb_info* ctbs;       // slice_idx (validated by the build) and slice_addr_rs per CTB
  const de265hip_slice_params* slices;
  const uint16_t* tile_id;             // per CTB
  uint8_t* flags;                      // blk_flags, w4 x h4: the low nibble is the host's, the high nibble is written here
  int32_t w4, h4, lc, lmincb, lt, cbs_w, tbs_w, ctbs_w, lf_across_tiles, pad;
};

// deblock.cc:175-207 (filterLeftCbEdge / filterTopCbEdge): the CB's own edge at x0 (vertical) or y0 (horizontal) is filtered
// unless it is the picture's edge, or a CTB edge that is a slice boundary the CB's slice does not filter across, or a tile
// boundary the picture does not filter across
EDGE_FN bool edge_cb_edge_filtered(const EdgeJob& J, int pos, int ctb_a, int nb, const de265hip_slice_params& sh)
{
  if (!pos) return false;
  if (pos & ((1 << J.lc) - 1)) return true;
  if (!sh.slice_loop_filter_across_slices_enabled_flag && J.ctbs[nb].slice_addr_rs != J.ctbs[ctb_a].slice_addr_rs) return false;
  if (!J.lf_across_tiles && J.tile_id[nb] != J.tile_id[ctb_a]) return false;
  return true;
}

// the edge bits (DE265HIP_BLK_EDGE_*) of unit (ux, uy).  Every read is bounded by the picture whatever the structure says (the
// build only checks that cb_log2 entries are 0 or in [lmincb, lc] and part modes are <= 7): a unit that no CB covers gets none,
// and the tree walk stops at MinTb.
EDGE_FN uint8_t edge_bits_of_unit(const EdgeJob& J, int ux, int uy)
{
  const int x = ux << 2, y = uy << 2;
  // 1. the covering CB: the one candidate origin, aligned to its own size, whose entry is that size (no early exit: the at most
  //    four loads are independent of each other and go out together)
  int lcb = 0, x0 = 0, y0 = 0;
  for (int s = J.lmincb; s <= J.lc; s++) {
    const int cx = (x >> s) << s, cy = (y >> s) << s;
    if (J.cb_log2[(cx >> J.lmincb) + (size_t)(cy >> J.lmincb) * J.cbs_w] == s && !lcb) { lcb = s; x0 = cx; y0 = cy; }
  }
  if (!lcb) return 0;
  const int ctb_a = (x0 >> J.lc) + (y0 >> J.lc) * J.ctbs_w;
  const de265hip_slice_params& sh = J.slices[J.ctbs[ctb_a].slice_idx];
  if (sh.slice_deblocking_filter_disabled_flag) return 0;            // deblock.cc:213
  // 2. the leaf TU: down the transform tree from the CB by the split bits (markTransformBlockBoundary)
  int tx = x0, ty = y0, ls = lcb;
  for (int d = 0; ls > J.lt; d++) {
    if (!((J.tu_split[(tx >> J.lt) + (size_t)(ty >> J.lt) * J.tbs_w] >> d) & 1)) break;
    ls--;
    const int h = 1 << ls;
    if (x >= tx + h) tx += h;
    if (y >= ty + h) ty += h;
  }
  // 3. TU edges; on the CB's own edges the CB rules
  uint8_t e = 0;
  if (x == tx && (x != x0 || edge_cb_edge_filtered(J, x0, ctb_a, ctb_a - 1, sh))) e |= DE265HIP_BLK_EDGE_TU_V;
  if (y == ty && (y != y0 || edge_cb_edge_filtered(J, y0, ctb_a, ctb_a - J.ctbs_w, sh))) e |= DE265HIP_BLK_EDGE_TU_H;
  // 4. PB edges (markPredictionBlockBoundary, deblock.cc:66-128, AMP included): the column / row of units the edge falls into
  const int h2 = 1 << (lcb - 1), q4 = 1 << (lcb - 2);
  int vx = -1, hy = -1;
  switch (J.cb_part[(x0 >> J.lmincb) + (size_t)(y0 >> J.lmincb) * J.cbs_w]) {
    case 1: hy = h2; break;            // PART_2NxN
    case 2: vx = h2; break;            // PART_Nx2N
    case 3: vx = h2; hy = h2; break;   // PART_NxN
    case 4: hy = q4; break;            // PART_2NxnU
    case 5: hy = h2 + q4; break;       // PART_2NxnD
    case 6: vx = q4; break;            // PART_nLx2N
    case 7: vx = h2 + q4; break;       // PART_nRx2N
    default: break;
  }
  if (vx >= 0 && ux == ((x0 + vx) >> 2)) e |= DE265HIP_BLK_EDGE_PB_V;
  if (hy >= 0 && uy == ((y0 + hy) >> 2)) e |= DE265HIP_BLK_EDGE_PB_H;
  return e;
}

// units [first, w4 * h4) in steps of `step`: the host's low nibble kept, the edge bits replaced, ONE whole-byte store per unit
EDGE_FN void edge_flags_units(const EdgeJob& J, long first, long step)
{
  const long n = (long)J.w4 * J.h4;
  for (long i = first; i < n; i += step) {
    const int ux = (int)(i % J.w4), uy = (int)(i / J.w4);
    J.flags[i] = (uint8_t)((J.flags[i] & 0x0F) | edge_bits_of_unit(J, ux, uy));
  }
}

}  // namespace d265
