// Prints chained block hashes of the native allocator for tests/test_lora_cpu.py: the hash of tokens
// 0..63 from parent 0, the hash of tokens 64..127 chained onto it, and the first hash from parent 77.
#include <cstdio>
#include <vector>

#include "block_allocator.h"

int main() {
  std::vector<int32_t> t(128);
  for (int i = 0; i < 128; ++i) t[i] = i;
  const uint64_t h0 = penny::block_hash(0, t.data(), 64);
  const uint64_t h1 = penny::block_hash(h0, t.data() + 64, 64);
  const uint64_t s0 = penny::block_hash(77, t.data(), 64);
  std::printf("%016llx %016llx %016llx\n", (unsigned long long)h0, (unsigned long long)h1, (unsigned long long)s0);
  return 0;
}
