// The lane contexts of the device kernels (hb_kernels.hip) and of the device unit wrappers (tests/gpu_unit/primitives.hip): what the
// lane-cooperative code of the hb_*.hpp headers is instantiated with on the GPU.  In an anonymous namespace, like everything
// else that is private to the translation unit that includes it.
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct DeviceCtx {
  int lane, nlanes;
  __device__ DeviceCtx() : lane(threadIdx.x), nlanes(blockDim.x) {}
  __device__ void sync() const { __syncthreads(); }
};
// Context of the kernels whose workgroup is exactly one wavefront and whose lanes exchange data through LDS only.  The
// LDS unit executes the DS instructions of one wave in order, so "every lane's earlier LDS writes are visible to every
// lane's later LDS reads" needs no hardware barrier and, unlike __syncthreads() (a workgroup-scope fence: s_waitcnt
// vmcnt(0)), does not drain the global loads / stores in flight — software-pipelined prefetches stay in flight across
// the phases of a stage.  What remains is a compiler-level ordering point.
struct WaveCtx {
  int lane;
  static constexpr int nlanes = 64;
  __device__ WaveCtx() : lane(threadIdx.x) {}
  __device__ explicit WaveCtx(int l) : lane(l) {}
  __device__ void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
};

}  // namespace
