// tuning.hip -- the one place the library reads its environment (tuning.h).
#include <cstdio>
#include <cstdlib>
#include "tuning.h"

namespace tf {
namespace {
bool flag(const char* name) { return getenv(name) != nullptr; }
long num(const char* name, long dflt) { const char* e = getenv(name); return e ? atol(e) : dflt; }
Tuning parse() {
  Tuning t;
  t.ew_blocks = (int)num("TINYFACES_EW_BLOCKS", 1024);
  t.ew_blocks_small = (int)num("TINYFACES_EW_BLOCKS_SMALL", 768);
  t.ew_small_mb = (int)num("TINYFACES_EW_SMALL_MB", 40);
  t.comm_fail_init = flag("TINYFACES_COMM_FAIL_INIT");
  t.comm_fail_bucket = (int)num("TINYFACES_COMM_FAIL_BUCKET", -1);
  t.conv3h_dbg = (int)num("TINYFACES_CONV3H_DBG", 0);
  t.single_stream = flag("TINYFACES_SINGLE_STREAM");
  t.dbg_skip_wgrad = flag("TINYFACES_DBG_SKIP_WGRAD");
  t.grad_memset_full = flag("TINYFACES_GRAD_MEMSET_FULL");
  t.dbg_group_refuse = flag("TINYFACES_DBG_GROUP_REFUSE");
  t.pool_stats_blocks = (int)num("TINYFACES_POOL_STATS_BLOCKS", 8192);
  t.profile_bracket = flag("TINYFACES_PROFILE_BRACKET");
  t.stem_wgrad_blocks = (int)num("TINYFACES_STEM_WGRAD_BLOCKS", 384);
  t.wgrad3_blocks = (int)num("TINYFACES_WGRAD3_BLOCKS", 128);
  t.wgrad3_dbg = (int)num("TINYFACES_WGRAD3_DBG", 0);
  t.wgrad_blocks = (int)num("TINYFACES_WGRAD_BLOCKS", 512);
  t.conv_dbg = (int)num("TF_CONV_DBG", 0);
  // modes that make results invalid say so, once
  if (t.conv3h_dbg) fprintf(stderr, "tinyfaces: TINYFACES_CONV3H_DBG=%d -- timing-ablation mode, convolution RESULTS ARE INVALID\n", t.conv3h_dbg);
  if (t.conv_dbg & 15) fprintf(stderr, "tinyfaces: TF_CONV_DBG=%d -- timing-ablation mode, convolution RESULTS ARE INVALID\n", t.conv_dbg);
  else if (t.conv_dbg) fprintf(stderr, "tinyfaces: TF_CONV_DBG=%d -- A/B form of the statistic epilogue (results unchanged)\n", t.conv_dbg);
  if (t.dbg_skip_wgrad) fprintf(stderr, "tinyfaces: TINYFACES_DBG_SKIP_WGRAD -- weight gradients NOT computed, timing only\n");
  if (t.wgrad3_dbg) fprintf(stderr, "tinyfaces: TINYFACES_WGRAD3_DBG=%d -- timing-ablation mode, weight gradients ARE INVALID\n", t.wgrad3_dbg);
  return t;
}
}  // namespace
const Tuning& tuning() {
  static const Tuning t = parse();
  return t;
}
}  // namespace tf
