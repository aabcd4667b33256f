// Host program for tests/test_batch_panda_runtime_cpu.py: the sizes and alignments of the entries of m3_batch_command's
// panda_env table as the library's own header defines them (csrc/m3_internal.hpp), so that the test types none of them in.
// Host side only:
//   hipcc --cuda-host-only -std=c++17 -I m3p2i_aip_amd/csrc batch_panda_entry_sizes.hip -o batch_panda_entry_sizes
// Prints: sizeof BatchPandaEntry, sizeof BatchPandaEntryRT, sizeof UpdateArgs, alignof BatchPandaEntry, alignof
// BatchPandaEntryRT, alignof UpdateArgs.
#include <cstdio>

#include "m3_internal.hpp"

int main() {
    static_assert(sizeof(m3::BatchPandaEntryRT) > sizeof(m3::BatchPandaEntry), "the run-time entry is the larger one");
    std::printf("%zu %zu %zu %zu %zu %zu\n", sizeof(m3::BatchPandaEntry), sizeof(m3::BatchPandaEntryRT), sizeof(m3::UpdateArgs),
                alignof(m3::BatchPandaEntry), alignof(m3::BatchPandaEntryRT), alignof(m3::UpdateArgs));
    return 0;
}
