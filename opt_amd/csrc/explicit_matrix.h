// explicit_matrix.h — the assembled block-CSR matrix behind ReducedSystem("explicit") (S) and
// NormalMatrix("explicit") (H = J^T J): the pattern with its per-block pair lists, the values
// and the per-instance buffers the numeric phase sums them from. Built symbolically once per
// wiring of the graphs — on the device (schur_pattern_dev.hip), or on the host (schur_pattern.h)
// under OPT_AMD_SYMBOLIC=host or where the device form's temporaries do not fit — and filled
// once per Step by the generated kernels, which GenericOp launches on buffers().
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>
#include "gen/codegen.h"
#include "plan.h"
#include "schur_pattern.h"
#include "schur_pattern_dev.h"

namespace optamd {

// What tells the two matrices apart in the symbolic phase and in the buffers' sizes.
struct ExplicitForm {
    const char* what;    // the matrix's name in messages
    bool distinct;       // only pairs of two different instances (schur_pattern.h)
    int C;               // block dimension
    int per_instance;    // values per edge instance in each per-instance buffer
    int buffers;         // per-instance buffers: 2 (W_q, Y_q of S) or 1 (G_q of H)
    int long_row;        // rows with more blocks go to the long-row list; 0: no such list
};

template <typename T>
class ExplicitMatrix {
public:
    // What the launches pass (by address: hipModuleLaunchKernel's argument list). Every pointer
    // is null until the first build; longRow stays null where the form has no long-row list.
    struct Buffers {
        int *rowPtr = nullptr, *colInd = nullptr, *blkRow = nullptr, *pairPtr = nullptr, *pairs = nullptr;
        int* longBlk = nullptr;   // blocks with more than gen::kSchurLongPairs pairs
        int* longRow = nullptr;   // rows with more than ExplicitForm::long_row blocks
        int nLong = 0, nLongRow = 0;
        struct QBase { long long b[16]; } qbase{};   // per instance list: its first position
        T* val = nullptr;
        T* inst[2] = {nullptr, nullptr};
        long long nnzb = 0;
    };

    ExplicitMatrix() = default;
    ExplicitMatrix(const ExplicitMatrix&) = delete;
    ExplicitMatrix& operator=(const ExplicitMatrix&) = delete;
    ~ExplicitMatrix() { release(); }

    const Buffers& buffers() const { return b_; }
    // no pattern yet, or one for an earlier wiring (generation: the owner's count of re-wirings)
    bool stale(unsigned long long generation) const { return !b_.rowPtr || generation_ != generation; }
    void release() {
        for (int** q : {&b_.rowPtr, &b_.colInd, &b_.blkRow, &b_.pairPtr, &b_.pairs, &b_.longBlk, &b_.longRow}) { dfree(*q); *q = nullptr; }
        for (T** q : {&b_.val, &b_.inst[0], &b_.inst[1]}) { dfree(*q); *q = nullptr; }
    }

    // The symbolic phase for `lists` (at most 16) over nE eliminated and nR retained elements,
    // then the values and per-instance buffers allocated for it.
    void build(const ExplicitForm& form, long long nE, long long nR, const std::vector<SchurListDev>& lists,
               unsigned long long generation, hipStream_t s) {
        release();   // the old wiring's buffers first: both need not fit together
        form_ = form;
        rows_ = nR;
        long long nq = 0;
        for (auto& l : lists) nq += l.n;
        const size_t per = (size_t)form.per_instance;
        try {
            if (mode_ == kHost || !build_device(nE, lists, (long long)(form.buffers * per * sizeof(T)) * nq, s))
                build_host(nE, lists, s);
        } catch (const std::length_error& e) {
            throw PlanError(std::string("generic: ") + e.what());
        }
        b_.val = (T*)dmalloc(sizeof(T) * std::max<size_t>(1, (size_t)form.C * form.C * b_.nnzb));
        for (int k = 0; k < form.buffers; ++k) b_.inst[k] = (T*)dmalloc(sizeof(T) * std::max<size_t>(1, per * nq_));
        generation_ = generation;
    }

    // block rows, block dimension, blocks; false before the first symbolic phase
    bool shape(long long* rows, int* dim, long long* nnzb) const {
        if (!b_.rowPtr) return false;
        if (rows) *rows = rows_;
        if (dim) *dim = form_.C;
        if (nnzb) *nnzb = b_.nnzb;
        return true;
    }
    void copy_out(int* rowPtr, int* colInd, T* val, hipStream_t s) const {
        OPT_HIP_CHECK(hipMemcpyAsync(rowPtr, b_.rowPtr, sizeof(int) * (rows_ + 1), hipMemcpyDefault, s));
        OPT_HIP_CHECK(hipMemcpyAsync(colInd, b_.colInd, sizeof(int) * b_.nnzb, hipMemcpyDefault, s));
        OPT_HIP_CHECK(hipMemcpyAsync(val, b_.val, sizeof(T) * b_.nnzb * form_.C * form_.C, hipMemcpyDefault, s));
    }
    // the buffers the captured PCG loop's SpMV bakes in (StencilPlan::pcg_graph_begin)
    void capture_key(std::vector<unsigned long long>* key) const {
        for (const void* q : {(const void*)b_.rowPtr, (const void*)b_.colInd, (const void*)b_.val, (const void*)b_.longRow})
            key->push_back((unsigned long long)(uintptr_t)q);
    }
    // what the last symbolic phase did (OptAMD_PlanSymbolicInfo); empty before the first
    const std::string& info() const { return info_; }
    long long pairs() const { return npairs_; }

private:
    // The pattern built in place from the device lists; false, with nothing allocated, where the
    // temporaries do not fit: that wiring takes the host path.
    bool build_device(long long nE, const std::vector<SchurListDev>& lists, long long reserve_bytes, hipStream_t s) {
        SchurPatternDev D;
        const char* cap = getenv("OPT_AMD_SYMBOLIC_MAX_BYTES");
        const bool built = schur_pattern_build_dev(nE, rows_, lists, form_.distinct, form_.what, gen::kSchurLongPairs,
                                                   form_.long_row, reserve_bytes, cap && *cap ? atoll(cap) : -1, s, &D);
        transient_ = D.transient_bytes;
        if (!built) return false;
        for (size_t l = 0; l < lists.size(); ++l) b_.qbase.b[l] = D.base[l];
        b_.nnzb = D.n_blocks;
        npairs_ = D.n_pairs;
        nq_ = D.n_instances;
        b_.rowPtr = D.rowPtr;
        b_.colInd = D.colInd;
        b_.blkRow = D.blkRow;
        b_.pairPtr = D.pairPtr;
        b_.pairs = D.pairs;
        b_.nLong = D.n_long;
        b_.longBlk = D.longBlk;
        if (form_.long_row > 0) {
            b_.nLongRow = D.n_longrow;
            b_.longRow = D.longRow;
        } else {
            dfree(D.longRow);
        }
        set_info("device", mode_ == kDevice ? "env" : "default");
        return true;
    }
    // The host builder: the lists' vertex arrays down (the edge's own number where a list has no
    // ev), the pattern and the long lists up.
    void build_host(long long nE, const std::vector<SchurListDev>& lists, hipStream_t s) {
        std::vector<std::vector<int>> ev(lists.size()), rv(lists.size());
        for (size_t l = 0; l < lists.size(); ++l) {
            const SchurListDev& L = lists[l];
            ev[l].resize(std::max<long long>(1, L.n));
            rv[l].resize(std::max<long long>(1, L.n));
            OPT_HIP_CHECK(hipMemcpyAsync(rv[l].data(), L.rv, sizeof(int) * L.n, hipMemcpyDeviceToHost, s));
            if (L.ev) OPT_HIP_CHECK(hipMemcpyAsync(ev[l].data(), L.ev, sizeof(int) * L.n, hipMemcpyDeviceToHost, s));
            else
                for (long long e = 0; e < L.n; ++e) ev[l][e] = (int)(L.ebase + e);
        }
        OPT_HIP_CHECK(hipStreamSynchronize(s));
        std::vector<SchurList> hl;
        for (size_t l = 0; l < lists.size(); ++l) hl.push_back({ev[l].data(), rv[l].data(), lists[l].n});
        SchurPattern P;
        schur_pattern_build(nE, rows_, hl, &P, form_.distinct, form_.what);
        for (size_t l = 0; l < P.base.size(); ++l) b_.qbase.b[l] = P.base[l];
        b_.nnzb = P.n_blocks();
        npairs_ = P.n_pairs();
        nq_ = P.n_instances;
        auto up = [&](const std::vector<int>& v) {
            int* d = (int*)dmalloc(sizeof(int) * std::max<size_t>(1, v.size()));
            if (!v.empty()) OPT_HIP_CHECK(hipMemcpyAsync(d, v.data(), sizeof(int) * v.size(), hipMemcpyHostToDevice, s));
            return d;
        };
        b_.rowPtr = up(P.rowPtr);
        b_.colInd = up(P.colInd);
        b_.blkRow = up(P.blkRow);
        b_.pairPtr = up(P.pairPtr);
        b_.pairs = up(P.pairs);
        std::vector<int> lng, lrow;   // blocks left to the assemble kernel's long form, rows to the SpMV's workgroup form
        for (long long b = 0; b < b_.nnzb; ++b)
            if (P.pairPtr[b + 1] - P.pairPtr[b] > gen::kSchurLongPairs) lng.push_back((int)b);
        b_.nLong = (int)lng.size();
        b_.longBlk = up(lng);
        if (form_.long_row > 0) {
            for (long long r = 0; r < rows_; ++r)
                if (P.rowPtr[r + 1] - P.rowPtr[r] > form_.long_row) lrow.push_back((int)r);
            b_.nLongRow = (int)lrow.size();
            b_.longRow = up(lrow);
        }
        OPT_HIP_CHECK(hipStreamSynchronize(s));   // (the host vectors go out of scope)
        if (mode_ == kHost) transient_ = 0;       // no device attempt was made
        set_info("host", mode_ == kHost ? "env" : "memory");
    }
    void set_info(const char* path, const char* reason) {
        info_ = std::string("path=") + path + " reason=" + reason + " pairs=" + std::to_string(npairs_) + " blocks=" +
                std::to_string(b_.nnzb) + " instances=" + std::to_string(nq_) + " transient_bytes=" + std::to_string(transient_);
    }

    // where the symbolic phase runs: OPT_AMD_SYMBOLIC=host|device, read when the plan is made
    // (unset: the device, and the host where its temporaries do not fit)
    enum { kDefault, kHost, kDevice };
    static int mode_from_env() {
        const char* v = getenv("OPT_AMD_SYMBOLIC");
        const std::string w = v ? v : "";
        return w == "host" ? kHost : w == "device" ? kDevice : kDefault;
    }
    const int mode_ = mode_from_env();
    ExplicitForm form_{};
    Buffers b_;
    long long rows_ = 0, npairs_ = 0, nq_ = 0;
    long long transient_ = 0;                // the device attempt's temporaries, of the last build
    unsigned long long generation_ = 0;      // the owner's generation the pattern was built for
    std::string info_;
};

}  // namespace optamd
