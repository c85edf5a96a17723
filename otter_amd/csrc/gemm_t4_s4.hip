// gemm_t4_s4.hip -- one translation unit for the two kernel families with fused full-tile tails: variant 26 (gemm_t4.hip) and the small-grid
// ring kernels, variants 25 / 30 (gemm_s4.hip).  Each file is complete by itself; they are compiled together because hipcc specialises the
// tail helpers they share (gemm_tail.h: tail_stripe_*, epilogue_stripe, block_partial) on the arguments of ALL their call sites in a unit before
// it inlines them: compiled apart, twelve instantiations of variant 26 and all eight ring kernels come out with other (not measured) object
// code than the one the timings in DESIGN.md and profiles/ belong to (tools/isa_equal.py; profiles/r21_gemm_split.txt).
#include "gemm_t4.hip"
#include "gemm_s4.hip"
