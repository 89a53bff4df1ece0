// tuning.h -- every run-time knob of the library in ONE struct, parsed from the environment ONCE (r6; rounds 1-5 had 64 getenv() calls spread
// over the kernel files, each behind its own function-local static).  tf::tuning() returns the parsed values; defaults are what the product runs.
// What qualifies as a knob: a block count or size threshold that a new ROCm may move (re-swept in r6); what a test sets, and the fault
// injections; a measurement switch (one stream, the bracket clock); an ablation mask that travels into a kernel as an argument.  An A/B switch
// whose question is answered does NOT: its losing arm is a row of DESIGN_HISTORY.md section 7 and the code takes the winner unconditionally.
// Invalid-result modes announce themselves on stderr once.
#pragma once
namespace tf {
struct Tuning {
  int ew_blocks = 1024;                  // TINYFACES_EW_BLOCKS: block cap of the fused BN passes (r6: 2048 -> 1024, +1.0 % on the step)
  int ew_blocks_small = 768;             // TINYFACES_EW_BLOCKS_SMALL: the cap for tensors below ew_small_mb
  int ew_small_mb = 40;                  // TINYFACES_EW_SMALL_MB
  bool comm_fail_init = false;           // TINYFACES_COMM_FAIL_INIT
  int comm_fail_bucket = -1;             // TINYFACES_COMM_FAIL_BUCKET
  int conv3h_dbg = 0;                    // TINYFACES_CONV3H_DBG
  bool single_stream = false;            // TINYFACES_SINGLE_STREAM
  bool dbg_skip_wgrad = false;           // TINYFACES_DBG_SKIP_WGRAD
  bool grad_memset_full = false;         // TINYFACES_GRAD_MEMSET_FULL
  bool dbg_group_refuse = false;         // TINYFACES_DBG_GROUP_REFUSE
  int pool_stats_blocks = 8192;          // TINYFACES_POOL_STATS_BLOCKS
  bool profile_bracket = false;          // TINYFACES_PROFILE_BRACKET
  int stem_wgrad_blocks = 384;           // TINYFACES_STEM_WGRAD_BLOCKS
  int wgrad3_blocks = 128;               // TINYFACES_WGRAD3_BLOCKS (r6: 256 -> 128 pixel slices x tiles: half the partial-tile traffic, +0.4 % on the step)
  int wgrad3_dbg = 0;                    // TINYFACES_WGRAD3_DBG
  int wgrad_blocks = 512;                // TINYFACES_WGRAD_BLOCKS
  int conv_dbg = 0;                      // TF_CONV_DBG
};
const Tuning& tuning();
}  // namespace tf
