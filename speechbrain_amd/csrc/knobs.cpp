// sbk_prof_set_knob / sbk_prof_get_knob: the one table from a key of include/sbk.h's enum sbk_knob to the switch it names.
#include "knobs.h"

#include <climits>

#include "sbk.h"

// the switch behind a key (nullptr: no such key)
static int* knob_slot(int key) {
  switch (key) {
    case SBK_KNOB_SKINNY_OFF: return &sbk::g_skinny_off;
    case SBK_KNOB_CROSS_ROWS: return &sbk::g_cross_rows;
    case SBK_KNOB_CROSS_FC256: return &sbk::g_cross_fc256;
    case SBK_KNOB_TILED_SPLITK: return &sbk::g_tiled_splitk;
    case SBK_KNOB_SK_MODE: return &sbk::g_sk_mode;
    case SBK_KNOB_SK_MIN_ROWS: return &sbk::g_sk_min_rows;
    case SBK_KNOB_X3_ROUTE_ROWS: return &sbk::g_x3_route_rows;
    case SBK_KNOB_X3_ROUTE_TILES: return &sbk::g_x3_route_tiles;
    case SBK_KNOB_SCORE_FUSED: return &sbk::g_score_fused;
    case SBK_KNOB_X3R_MODE: return &sbk::g_x3r_mode;
    case SBK_KNOB_X3R_MIN_ROWS: return &sbk::g_x3r_min_rows;
    case SBK_KNOB_X3R_LN: return &sbk::g_x3r_ln;
    case SBK_KNOB_PERSIST: return &sbk::g_persist;
    case SBK_KNOB_PERSIST_GRID: return &sbk::g_persist_grid;
    case SBK_KNOB_PERSIST_STAMPS: return &sbk::g_persist_stamps;
    case SBK_KNOB_X3R_XC: return &sbk::g_x3r_xc;
    case SBK_KNOB_NT_MASK: return &sbk::g_nt_mask;
    case SBK_KNOB_SELF_ANC: return &sbk::g_self_anc;
    case SBK_KNOB_X3R_PAIR: return &sbk::g_x3r_pair;
    case SBK_KNOB_PERSIST_TREE: return &sbk::g_persist_tree;
    case SBK_KNOB_ATTN_EXP2: return &sbk::g_attn_exp2;
    case SBK_KNOB_LP256: return &sbk::g_lp256;
    case SBK_KNOB_X3P_FAST_EPI: return &sbk::g_x3p_fast_epi;
    default: return nullptr;
  }
}
extern "C" void sbk_prof_set_knob(int key, int value) {
  if (int* p = knob_slot(key)) *p = value;
}
extern "C" int sbk_prof_get_knob(int key) {
  const int* p = knob_slot(key);
  return p ? *p : INT_MIN;
}
