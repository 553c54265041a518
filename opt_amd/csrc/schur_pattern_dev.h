// schur_pattern_dev.h — the symbolic phase of the explicitly formed S and H on the device
// (schur_pattern_dev.hip): schur_pattern_build's contract (schur_pattern.h) with device arrays in
// and out, every array equal to the host builder's element for element.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "schur_pattern.h"

namespace optamd {

// One instance list on the device. ev == nullptr (the `distinct` form): edge e's "eliminated
// vertex" is ebase + e and the list order is the identity. order, where given, is the edges in
// the stable order by ev (GenArgs::geid of the eliminated slot); without it the builder sorts.
struct SchurListDev {
    const int* ev;
    const int* rv;
    const int* order;
    long long n;
    long long ebase;
};

struct SchurPatternDev {
    long long n_instances = 0, n_pairs = 0, n_blocks = 0;
    std::vector<long long> base;   // per list: its first position
    int n_long = 0, n_longrow = 0;
    // dmalloc'd (never null after a build); the caller owns them
    int *rowPtr = nullptr, *colInd = nullptr, *blkRow = nullptr, *pairPtr = nullptr, *pairs = nullptr;
    int *longBlk = nullptr;    // blocks with more than long_pairs pairs, ascending
    int *longRow = nullptr;    // rows with more than long_row blocks, ascending (long_row > 0)
    long long transient_bytes = 0;   // the temporaries' footprint, set on a refusal too
    void release();
};

// Builds the pattern on `stream`. long_row <= 0: no long-row list.
// reserve_bytes: what the caller allocates next to the pattern; max_bytes >= 0 caps the
// temporaries (OPT_AMD_SYMBOLIC_MAX_BYTES). Returns false, with nothing allocated, when the
// temporaries exceed max_bytes, or free device memory less the pattern and reserve_bytes, or
// when the instances alone exceed 2^31 - 1 (the host builder words that refusal). Throws the
// host builder's std::length_error for more than 2^31 - 1 pairs or blocks.
bool schur_pattern_build_dev(long long nE, long long nR, const std::vector<SchurListDev>& lists, bool distinct,
                             const char* what, int long_pairs, int long_row, long long reserve_bytes,
                             long long max_bytes, hipStream_t stream, SchurPatternDev* out);

// Host arrays in, host arrays out (OptAMD_SchurPatternDevice / OptAMD_NormalPatternDevice): the
// lists uploaded, the pattern built on the current device's null stream and downloaded. In the
// `distinct` form lists[l].ev holds ebase + e as schur_pattern_build takes it.
void schur_pattern_build_dev_host(long long nE, long long nR, const std::vector<SchurList>& lists, bool distinct,
                                  const char* what, SchurPattern* out);

}  // namespace optamd
