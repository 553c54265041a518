// schur_pattern.h — symbolic phase of the explicitly formed Schur complement (host only, no
// device code): from the graphs' vertex arrays alone, the block-CSR pattern of
// S = B - E M^-1 E^T over the retained elements and, per block, the ordered list of instance
// pairs whose products sum into it (gen/codegen_schur_explicit.cpp: gen_schur_assemble).
//
// An instance list is one (eliminated slot, retained slot) pair of one graph: ev[e] / rv[e] are
// edge e's eliminated / retained vertex. Within a list the instances are the edges in the
// eliminated slot's incidence order (by eliminated vertex, ties by edge id: a stable sort, the
// order of GenArgs::goff / geid), and instance i of list l has position q = base_l + i, base_l
// the sum of the earlier lists' edge counts. For every eliminated vertex p, every ordered pair
// (q1, q2) of instances at p — over all lists, duplicates of one (retained, eliminated) pair
// included — goes to block (retained vertex of q1, retained vertex of q2). Blocks are sorted by
// (row, column); within a block the pairs keep the enumeration order (p ascending, then q1, then
// q2 in the order [list, position]): two stable counting sorts, O(pairs + elements). Every
// retained element's diagonal block is present, with an empty list if need be (it holds B).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace optamd {

struct SchurList {
    const int* ev;   // per edge: vertex in the eliminated space
    const int* rv;   // per edge: vertex in the retained space
    long long n;     // edges
};

struct SchurPattern {
    long long n_instances = 0;        // positions q
    std::vector<long long> base;      // per list: its first position
    std::vector<int> rowPtr;          // nR + 1
    std::vector<int> colInd;          // per block, ascending inside a row
    std::vector<int> blkRow;          // per block: its row
    std::vector<int> pairPtr;         // nnzb + 1
    std::vector<int> pairs;           // 2 per pair: q1, q2
    long long n_pairs() const { return (long long)pairs.size() / 2; }
    long long n_blocks() const { return (long long)colInd.size(); }
};

// nE / nR: elements of the eliminated / retained space (every vertex must lie inside; the
// plan has checked that). Throws std::length_error, naming the counts, when the instances,
// pairs or blocks exceed 2^31 - 1 (the pair count is known before anything of that size is
// allocated).
//
// `distinct` (the explicitly formed J^T J of NormalMatrix("explicit"), codegen_normal.cpp): the
// "eliminated vertex" is the graph edge itself (ev[e] = the edge's number among all graphs'
// edges), a list is one slot over the unknowns' space, and only the pairs of two DIFFERENT
// instances are listed: an instance's product with itself is part of the diagonal blocks the
// J^T F kernels leave. what: the matrix's name in the error message.
inline void schur_pattern_build(long long nE, long long nR, const std::vector<SchurList>& lists, SchurPattern* out,
                                bool distinct = false, const char* what = "explicit Schur complement") {
    SchurPattern& S = *out;
    S = SchurPattern();
    long long nq = 0;
    for (auto& l : lists) {
        S.base.push_back(nq);
        nq += l.n;
    }
    S.n_instances = nq;
    // instances by eliminated vertex: counts, offsets, then the retained vertex and position
    // of each, list after list, each list in its stable incidence order
    std::vector<long long> off(nE + 1, 0);
    for (auto& l : lists)
        for (long long e = 0; e < l.n; ++e) ++off[l.ev[e] + 1];
    for (long long p = 0; p < nE; ++p) off[p + 1] += off[p];
    std::vector<int> iq(nq), ir(nq);
    {
        std::vector<long long> fill(off.begin(), off.end() - 1);
        for (size_t li = 0; li < lists.size(); ++li) {
            const SchurList& l = lists[li];
            // position inside the list = rank in the stable sort by eliminated vertex
            std::vector<long long> lo(nE + 1, 0);
            for (long long e = 0; e < l.n; ++e) ++lo[l.ev[e] + 1];
            for (long long p = 0; p < nE; ++p) lo[p + 1] += lo[p];
            for (long long e = 0; e < l.n; ++e) {
                const int p = l.ev[e];
                const long long at = fill[p]++;
                iq[at] = (int)(S.base[li] + lo[p]++);
                ir[at] = l.rv[e];
            }
        }
    }
    long long np = 0;
    for (long long p = 0; p < nE; ++p) {
        const long long k = off[p + 1] - off[p];
        np += distinct ? k * (k - 1) : k * k;
    }
    const long long kMax = 2147483647LL;
    if (np > kMax || nq > kMax)
        throw std::length_error(std::string(what) + ": " + std::to_string(np) + " instance pairs over " +
                                std::to_string(nq) + " edge instances (at most 2^31 - 1 of each)");
    // pairs in enumeration order, then stable counting sorts by column and by row
    std::vector<int> pr(np), pc(np), p1(np), p2(np);
    {
        long long at = 0;
        for (long long p = 0; p < nE; ++p)
            for (long long x = off[p]; x < off[p + 1]; ++x)
                for (long long y = off[p]; y < off[p + 1]; ++y) {
                    if (distinct && x == y) continue;
                    pr[at] = ir[x]; pc[at] = ir[y]; p1[at] = iq[x]; p2[at] = iq[y];
                    ++at;
                }
    }
    std::vector<int> order(np), tmp(np);
    auto counting = [&](const std::vector<int>& key, const std::vector<int>& in, std::vector<int>& outv, bool first) {
        std::vector<long long> c(nR + 1, 0);
        for (long long i = 0; i < np; ++i) ++c[key[first ? i : in[i]] + 1];
        for (long long r = 0; r < nR; ++r) c[r + 1] += c[r];
        for (long long i = 0; i < np; ++i) {
            const int src = first ? (int)i : in[i];
            outv[c[key[src]]++] = src;
        }
    };
    counting(pc, tmp, tmp, true);       // tmp: pair ids by column
    counting(pr, tmp, order, false);    // order: by (row, column), enumeration order inside
    // blocks: runs of equal (row, column), the diagonal inserted where no pair lands on it
    S.rowPtr.assign(nR + 1, 0);
    S.pairs.resize(2 * np);
    long long i = 0;
    for (long long r = 0; r < nR; ++r) {
        S.rowPtr[r] = (int)S.colInd.size();
        bool diag = false;
        auto open = [&](int col) {
            if ((long long)S.colInd.size() >= kMax)
                throw std::length_error(std::string(what) + ": more than 2^31 - 1 blocks (" + std::to_string(np) +
                                        " instance pairs)");
            S.colInd.push_back(col);
            S.blkRow.push_back((int)r);
            S.pairPtr.push_back((int)i);
        };
        while (i < np && pr[order[i]] == r) {
            const int col = pc[order[i]];
            if (!diag && col > r) { open((int)r); diag = true; }
            if (col == r) diag = true;
            open(col);
            for (; i < np && pr[order[i]] == r && pc[order[i]] == col; ++i) {
                S.pairs[2 * i] = p1[order[i]];
                S.pairs[2 * i + 1] = p2[order[i]];
            }
        }
        if (!diag) open((int)r);
    }
    S.rowPtr[nR] = (int)S.colInd.size();
    S.pairPtr.push_back((int)np);
}

}  // namespace optamd
