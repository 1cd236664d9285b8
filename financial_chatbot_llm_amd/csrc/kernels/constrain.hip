// Token-automaton constraint tables (constrained tool-call decoding, agent/automaton.py).
//
// A byte-level DFA over the decide step's output language (byte_next[S, 256], 0xFFFF = dead) becomes
// a per-state TOKEN mask: bit t of masks[s, :] is set when walking token t's bytes from state s never
// dies.  Tokens without bytes (specials, ids past the tokenizer's vocabulary) are never allowed,
// except eot in accepting states (the done state is accepting too).  The sampler (sampler.hip,
// MASKED) then reads one mask byte per 8 logits.  Built once per automaton: S x V walks (about
// 2k x 128k for the two-tool automaton), one wave per 64 tokens of one state -- the lanes' verdicts
// are balloted into two mask words that lane 0 stores.
#include "common.h"

// grid (ceil(W / 2 / 4), S), 256 threads: wave w of block x scans tokens [64 g, 64 g + 64), g = 4 x + w.
// W (words per state) is a multiple of 4, so the W / 2 groups cover every word; bits >= V stay 0.
__global__ void __launch_bounds__(256) fsm_build_masks_kernel(const unsigned short* __restrict__ byte_next,
                                                              const unsigned char* __restrict__ accept,
                                                              const int* __restrict__ tok_off,
                                                              const unsigned char* __restrict__ tok_bytes,
                                                              uint32_t* __restrict__ masks, int S, int s0, int V,
                                                              int W, int eot) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int s = s0 + blockIdx.y, g = blockIdx.x * 4 + wid;
  if (g >= W / 2) return;                                 // wave-uniform
  const int t = g * 64 + lane;
  bool ok = false;
  if (t < V) {
    const int b0 = tok_off[t], b1 = tok_off[t + 1];
    if (b1 > b0) {
      int cur = s;
      ok = true;
      for (int j = b0; j < b1; ++j) {
        cur = byte_next[(size_t)cur * 256 + tok_bytes[j]];
        if (cur >= S) {                                   // dead (a live target is a state of the table)
          ok = false;
          break;
        }
      }
    } else {
      ok = t == eot && accept[s] != 0;
    }
  }
  const unsigned long long m = __ballot(ok);
  if (lane == 0) {
    uint32_t* row = masks + (size_t)s * W;
    row[2 * g] = (uint32_t)m;
    row[2 * g + 1] = (uint32_t)(m >> 32);
  }
}

// masks[s0 .. s0 + n) of a table of S states (byte_next / accept are the WHOLE table: transitions
// hold global state ids); tok_off[V + 1], W = ceil(V / 32) rounded up to a multiple of 4.
PENNY_API int penny_fsm_build_masks(const unsigned short* byte_next, const unsigned char* accept, const int* tok_off,
                                    const unsigned char* tok_bytes, unsigned int* masks, int S, int s0, int n, int V,
                                    int W, int eot, hipStream_t stream) {
  if (n <= 0) return 0;
  if (!byte_next || !accept || !tok_off || !tok_bytes || !masks || s0 < 0 || s0 + n > S || S >= 0xFFFF || V <= 0 ||
      W % 4 != 0 || (long)W * 32 < V || n > 65535)
    return (int)hipErrorInvalidValue;
  const int groups = W / 2;
  hipLaunchKernelGGL(fsm_build_masks_kernel, dim3((groups + 3) / 4, n), dim3(256), 0, stream, byte_next, accept,
                     tok_off, tok_bytes, masks, S, s0, V, W, eot);
  PENNY_RETURN_LAUNCH();
}
