// The tuning / measurement switches behind sbk_prof_set_knob (keys and meanings: enum sbk_knob of include/sbk.h; key -> variable:
// knobs.cpp).  Each is DEFINED in its kernel's file, next to the measurements that justify its default.
#pragma once

namespace sbk {
extern int g_skinny_off, g_tiled_splitk, g_sk_mode, g_sk_min_rows, g_x3_route_rows, g_x3_route_tiles;  // gemm.hip
extern int g_x3r_mode, g_x3r_min_rows, g_x3r_ln, g_x3r_xc, g_x3r_pair;                                // gemm_x3r.hip
extern int g_x3p_fast_epi;                                                                            // gemm_x3p.hip
extern int g_lp256;                                                                                   // gemm_lp256.hip
extern int g_cross_rows, g_cross_fc256, g_nt_mask, g_self_anc;                                        // decoder.hip
extern int g_persist, g_persist_grid, g_persist_stamps, g_persist_tree;                               // decoder_persist.hip
extern int g_score_fused;                                                                             // search.hip
extern int g_attn_exp2;                                                                               // relpos_attn.hip
}  // namespace sbk
