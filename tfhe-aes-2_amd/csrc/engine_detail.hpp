// What the translation units that implement Engine share (kernels.hip: the generic TFHE stages and the Engine
// core; aes_engine.hip: the AES application layer).  Internal: nothing outside csrc/*.hip includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine.hpp"

namespace tae {

#define HIPC(x) hip_check((x), #x)

constexpr int kThreads = 256;

inline unsigned grid_for(size_t total) { return (unsigned)std::min<size_t>((total + kThreads - 1) / kThreads, 65536); }

// dst[r * dst_stride + j] = src[r * src_stride + j]: rows of a key table gathered into a batch or scattered back,
// the bits of extract_bits interleaved into its output
static __global__ void copy_rows_strided_kernel(const uint64_t *__restrict__ src, size_t src_stride,
                                                uint64_t *__restrict__ dst, size_t dst_stride, size_t rows, size_t len) {
    const size_t total = rows * len;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t r = t / len, j = t - r * len;
        dst[r * dst_stride + j] = src[r * src_stride + j];
    }
}

template <class F>
void Engine::timed(int stage, F fn) {
    if (!timing_) {
        fn();
        return;
    }
    Span sp{next_event(), next_event(), stage};
    HIPC(hipEventRecord(sp.a, stream_));
    fn();
    HIPC(hipEventRecord(sp.b, stream_));
    spans_.push_back(sp);
}

}  // namespace tae
