// Per-slice class histogram of a label volume: what a continual-learning stage needs before it trains.  Its column sums are the
// per-class pixel counts behind the focal loss's class weights (universal_train.py:1006-1015, one (labels == c).sum().item() per
// class and batch there), and "column c of slice n is non-zero" is the slice list of PositiveSamplingDataset (:204-211, one
// torch.unique per decoded sample there).
//   cswin_class_counts  counts[n][c] = |{e : class(labels[n][e]) == c}| for c < ncls, counts[n][ncls] = the elements without a
//                       class; every row sums to slice_elems.  class(r) = r, or label_map[r] for 0 <= r < nmap; anything outside
//                       the map or mapped outside [0, ncls) has no class.
// Integer LDS atomics and plain stores only: no memset, no workspace, no global atomics, the same bits on every run.
#include "common.h"

// 1: a wave whose labels of one step are all the same value makes one addition (the measured form); 0: per-lane LDS
// atomics only, the form it is measured against (tools/continual_eval_time.py --plain-lib)
#ifndef CSWIN_CLASS_COUNTS_FAST
#define CSWIN_CLASS_COUNTS_FAST 1
#endif

namespace {

constexpr int CC_MAX_CLS = 256;
constexpr int CC_BINS = CC_MAX_CLS + 1;
constexpr int CC_WAVES = 4;

// bin of a raw id that may be anything (int64 labels: negative, beyond 2^32)
__device__ __forceinline__ int cc_bin(long long r, const int* __restrict__ map, int nmap, int ncls) {
    if (map) {
        if ((unsigned long long)r >= (unsigned long long)nmap) return ncls;
        r = map[r];
    }
    return (unsigned long long)r < (unsigned long long)ncls ? (int)r : ncls;
}

// One 256-thread workgroup per slice.  Each wave owns a uint32 histogram of ncls + 1 bins in LDS (a bin holds at most
// slice_elems < 2^31); lut[r] is the bin of raw id r < 256, made once per workgroup, so a uint8 label costs one LDS read and the
// map is never gathered from memory in the loop (int64 ids >= 256 take cc_bin).  A lane loads 16 B: 16 uint8 or 2 int64 labels.
// The slice's first element may sit anywhere (slices are densely packed): the elements before the first 16-B boundary and
// those after the last full vector are counted one per thread.
// Labels are long runs of one class, and 64 lanes adding to one LDS word serialise.  So a lane first compares its vector with
// the broadcast of its first element; if the whole wave holds one value (vote against the first lane's) a single lane adds
// the wave's element count to that bin.  Otherwise a lane whose own vector is one value adds its count, and the others add
// their elements one by one.
template <int BYTES>
__global__ __launch_bounds__(256) void class_counts_kernel(const unsigned char* __restrict__ labels, const int* __restrict__ map,
                                                           int nmap, long long* __restrict__ counts, long long slice_elems,
                                                           int ncls) {
    constexpr int VEC = 16 / BYTES;
    __shared__ unsigned hist[CC_WAVES][CC_BINS];
    __shared__ unsigned short lut[256];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int c = tid; c < CC_WAVES * CC_BINS; c += 256) (&hist[0][0])[c] = 0u;
    lut[tid] = (unsigned short)cc_bin(tid, map, nmap, ncls);
    __syncthreads();

    unsigned* __restrict__ my = hist[wave];
    const unsigned char* __restrict__ base = labels + (long long)blockIdx.x * slice_elems * BYTES;
    auto bin_of = [&](long long r) -> int { return (unsigned long long)r < 256ull ? (int)lut[r] : cc_bin(r, map, nmap, ncls); };
    auto element = [&](long long e) -> long long {
        if constexpr (BYTES == 1) return base[e];
        else return reinterpret_cast<const long long*>(base)[e];
    };

    const long long head = min((long long)(((16 - ((uintptr_t)base & 15)) & 15) / BYTES), slice_elems);
    const long long nvec = (slice_elems - head) / VEC;
    const long long tail0 = head + nvec * VEC;
    if (tid < head) atomicAdd(&my[bin_of(element(tid))], 1u);
    if (tail0 + tid < slice_elems) atomicAdd(&my[bin_of(element(tail0 + tid))], 1u);

    const u32x4* __restrict__ vecs = reinterpret_cast<const u32x4*>(base + head * BYTES);
    for (long long v0 = wave * 64; v0 < nvec; v0 += 256) {          // the trip count is the wave's: every lane votes
        const bool act = v0 + lane < nvec;
        u32x4 x = {0u, 0u, 0u, 0u};
        if (act) x = vecs[v0 + lane];
        long long first;
        bool one;                                                       // the lane's labels are all `first`
        if constexpr (BYTES == 1) {
            first = x.x & 0xFFu;
            const unsigned splat = (unsigned)first * 0x01010101u;
            one = x.x == splat && x.y == splat && x.z == splat && x.w == splat;
        } else {
            first = (long long)((unsigned long long)x.x | (unsigned long long)x.y << 32);
            one = x.x == x.z && x.y == x.w;
        }
#if CSWIN_CLASS_COUNTS_FAST
        const unsigned lo0 = __builtin_amdgcn_readfirstlane((unsigned)first);          // lane 0 is active whenever any lane is
        const unsigned hi0 = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)first >> 32));
        const long long first0 = (long long)((unsigned long long)lo0 | (unsigned long long)hi0 << 32);
        const unsigned long long active = __ballot(act);
        const unsigned long long agree = __ballot(act && one && first == first0);
        if (agree == active) {
            if (lane == 0) atomicAdd(&my[bin_of(first0)], (unsigned)(VEC * __popcll(active)));
            continue;
        }
        const bool lane_one = one;
#else
        const bool lane_one = false;
#endif
        if (act && lane_one) atomicAdd(&my[bin_of(first)], (unsigned)VEC);
        else if (act) {
            if constexpr (BYTES == 1) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int s = 0; s < 32; s += 8) atomicAdd(&my[lut[(x[q] >> s) & 0xFFu]], 1u);
            } else {
                atomicAdd(&my[bin_of(first)], 1u);
                atomicAdd(&my[bin_of((long long)((unsigned long long)x.z | (unsigned long long)x.w << 32))], 1u);
            }
        }
    }
    __syncthreads();
    long long* __restrict__ row = counts + (long long)blockIdx.x * (ncls + 1);
    for (int c = tid; c <= ncls; c += 256) row[c] = (long long)hist[0][c] + hist[1][c] + hist[2][c] + hist[3][c];
}

}  // namespace

extern "C" {

int cswin_class_counts(const void* labels, int label_bytes, const int* label_map, int nmap, long long* counts, int N,
                       long long slice_elems, int ncls, void* stream) {
    CSWIN_REQUIRE(labels && counts, CSWIN_ERR_SHAPE, "class_counts: null argument");
    CSWIN_REQUIRE(label_bytes == 1 || label_bytes == 8, CSWIN_ERR_UNSUPPORTED, "class_counts: label_bytes=%d (1 = uint8, 8 = int64)",
                  label_bytes);
    CSWIN_REQUIRE(ncls >= 1 && ncls <= CC_MAX_CLS, CSWIN_ERR_SHAPE, "class_counts: ncls=%d outside 1..%d", ncls, CC_MAX_CLS);
    CSWIN_REQUIRE(N >= 1 && slice_elems >= 1 && slice_elems <= 0x7FFFFFFFll, CSWIN_ERR_SHAPE,
                  "class_counts: N=%d slices of %lld elements (N >= 1, 1..2^31-1 elements)", N, slice_elems);
    CSWIN_REQUIRE(label_map ? nmap >= 1 : nmap == 0, CSWIN_ERR_SHAPE, "class_counts: nmap=%d %s a label map", nmap,
                  label_map ? "with" : "without");
    CSWIN_REQUIRE((uintptr_t)labels % (uintptr_t)label_bytes == 0 && (uintptr_t)counts % 8 == 0 && (uintptr_t)label_map % 4 == 0,
                  CSWIN_ERR_ALIGN, "class_counts: a pointer is not aligned to its element size");
    const unsigned char* l8 = static_cast<const unsigned char*>(labels);
    hipStream_t st = (hipStream_t)stream;
    if (label_bytes == 1) hipLaunchKernelGGL(class_counts_kernel<1>, dim3(N), dim3(256), 0, st, l8, label_map, nmap, counts, slice_elems, ncls);
    else hipLaunchKernelGGL(class_counts_kernel<8>, dim3(N), dim3(256), 0, st, l8, label_map, nmap, counts, slice_elems, ncls);
    CSWIN_LAUNCH_CHECK();
    return CSWIN_OK;
}

}  // extern "C"
