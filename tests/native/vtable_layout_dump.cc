// tests/test_vtable.py: the layout and slot types of a struct acceleration_functions as text - "sizeof <n>", one line
// "<slot> <offset> <type>" per slot and "entry <type>" for the init function (type = typeid name: equal strings for
// identical types only, so equal lines say what vtable_layout_check.cc's assignments in both directions say).
// Built against include/de265_hip_vtable.h it describes the product's mirror; built with -DAGAINST_REFERENCE against the
// reference's acceleration.h + fallback.h it describes libde265's own struct: tools/ref_source_golden.py writes that
// output to tests/golden/ref_vtable_layout.txt.
#include <cstddef>
#include <cstdio>
#include <typeinfo>
#ifdef AGAINST_REFERENCE
#include "acceleration.h"
#include "fallback.h"
typedef acceleration_functions S;
#define ENTRY init_acceleration_functions_fallback
#else
#include "de265_hip_vtable.h"
typedef de265hip_acceleration_functions S;
#define ENTRY init_acceleration_functions_hip
#endif

#define SLOT(s) printf("%s %zu %s\n", #s, offsetof(S, s), typeid(decltype(S::s)).name())
int main()
{
  printf("sizeof %zu\n", sizeof(S));
  SLOT(put_weighted_pred_avg_8); SLOT(put_unweighted_pred_8); SLOT(put_weighted_pred_8); SLOT(put_weighted_bipred_8);
  SLOT(put_weighted_pred_avg_16); SLOT(put_unweighted_pred_16); SLOT(put_weighted_pred_16); SLOT(put_weighted_bipred_16);
  SLOT(put_hevc_epel_8); SLOT(put_hevc_epel_h_8); SLOT(put_hevc_epel_v_8); SLOT(put_hevc_epel_hv_8); SLOT(put_hevc_qpel_8);
  SLOT(put_hevc_epel_16); SLOT(put_hevc_epel_h_16); SLOT(put_hevc_epel_v_16); SLOT(put_hevc_epel_hv_16); SLOT(put_hevc_qpel_16);
  SLOT(transform_bypass); SLOT(transform_bypass_rdpcm_v); SLOT(transform_bypass_rdpcm_h);
  SLOT(transform_skip_8); SLOT(transform_skip_rdpcm_v_8); SLOT(transform_skip_rdpcm_h_8);
  SLOT(transform_4x4_dst_add_8); SLOT(transform_add_8); SLOT(transform_skip_16); SLOT(transform_4x4_dst_add_16); SLOT(transform_add_16);
  SLOT(rotate_coefficients); SLOT(transform_idst_4x4); SLOT(transform_idct_4x4); SLOT(transform_idct_8x8); SLOT(transform_idct_16x16);
  SLOT(transform_idct_32x32); SLOT(add_residual_8); SLOT(add_residual_16); SLOT(rdpcm_v); SLOT(rdpcm_h); SLOT(transform_skip_residual);
  SLOT(fwd_transform_4x4_dst_8); SLOT(fwd_transform_8); SLOT(hadamard_transform_8);
  printf("entry %s\n", typeid(decltype(&ENTRY)).name());
  return 0;
}
