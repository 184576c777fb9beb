// Run-time switches of the library.  The environment is read ONCE per process, by sifsr_switches() in engine.hip -- the only reader of
// the environment in csrc/.  Parsing: unset -> default, otherwise atoi() of the value (so an unparsable value reads as 0).  Each switch selects other
// kernels or another schedule for the same maths and is exercised by tests/test_switches_gpu.py.
//
//   name (default)              values            what it selects
//   SIFSR_WGRAD_STREAM (1)      0 / non-zero      non-zero: weight gradients on a second, lower-priority stream (sifsr_engine_set_wgrad_stream overrides)
//   SIFSR_WGRAD_WINO (2)        1 / 2 / other     Winograd-domain weight gradients: 2 every layer, 1 up to 32 output channels, other: tap domain (and no fused 16 -> 16 kernel)
//   SIFSR_NO_WINO (0)           0 / non-zero      non-zero: direct forward / input-gradient kernels everywhere
//   SIFSR_NO_WINO8 (0)          0 / non-zero      non-zero: conv_mfma.hip's producer / consumer Winograd kernels instead of conv_wino8.hip's
//   SIFSR_NO_BWD16 (0)          0 / non-zero      non-zero: separate input- / weight-gradient kernels instead of the fused 16 -> 16 kernel (conv_bwd16.hip)
//   SIFSR_TAIL_APPLY (0)        0 / non-zero      non-zero: the outlay backward keeps its separate second pass (tail_bwd_apply)
//   SIFSR_HEAD_LINEAR (0)       0 / non-zero      non-zero: the first layer's weight gradient in its linear (Gram-matrix) form; measured slower
//   SIFSR_BF16_BWD16 (0)        0 / non-zero      non-zero: the bf16 mode also runs the fused 16 -> 16 kernel; measured slower
//   SIFSR_DBG_EARLY_REDUCE (3)  1 / 2 / 3 / other slab reductions on the second stream: 3 per encoder stage, 2 after the decoder + before db1, 1 before db1, other: one batch at the end
//   SIFSR_DBG_POOL_ON_LOAD (1)  0 / non-zero      non-zero: the fused kernel of inbloc.bloc.3 adds the pooling adjoint while staging; 0: the BatchNorm-backward reduction writes it back
#pragma once

struct Switches {
  int wgrad_stream, wgrad_wino, no_wino, no_wino8, no_bwd16, tail_apply, head_linear, bf16_bwd16, early_reduce, pool_on_load;
};
const Switches& sifsr_switches();   // immutable after the first call (function-local static)
