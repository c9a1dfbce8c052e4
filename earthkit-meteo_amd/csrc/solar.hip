// Solar geometry on gfx950: cosine of the solar zenith angle, its time average and the top-of-atmosphere incident
// radiation at every grid point.
// Reference: solar/array/solar.py:51-96, :99-179, :182-254.
//
// One kernel, one lane per point, no LDS.  The three functions of the reference are the same sum over time nodes (the
// instantaneous one has a single node with w = isr = 1); the node records -- five doubles per node, made on the host as
// the reference makes its dates, weights, declinations and time corrections -- are indexed by a wave-uniform loop
// counter off a kernel-argument pointer, so they arrive through the scalar cache, not as one vector load per lane.
// A point reads lat and lon once (4 or 8 B each; an operand that is a scalar or a vector along one axis of the result
// is indexed, never expanded), pays one sine/cosine pair for each, keeps the accumulator in a register through all
// nodes and writes once: 16 B read + 8 B written per point in f64.  T is the input dtype; all arithmetic is double on
// the upcast inputs and Out is rounded once at the end.  The per-point arithmetic is solar_point.hpp, shared with the
// host twin.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/ekm_thermo.h"
#include "map_kernel.hpp"
#include "solar_point.hpp"

namespace ekm {

constexpr int kSolarThreads = 256;

static_assert(EKM_SCALAR == 1 && EKM_LEVEL_MAJOR == 2 && EKM_LEVEL_MINOR == 3, "solar_point.hpp::solar_fetch and the header disagree");

template <class T, class Out>
__global__ __launch_bounds__(kSolarThreads) void solar_points(const SolarOperand<T> lat, const SolarOperand<T> lon,
                                                              const double* __restrict__ nodes, unsigned nnodes,
                                                              unsigned long long n, int small, Out* __restrict__ out) {
  const unsigned long long p = (unsigned long long)blockIdx.x * kSolarThreads + threadIdx.x;
  if (p >= n) return;
  const double la = solar_fetch<T>(lat, p, small != 0), lo = solar_fetch<T>(lon, p, small != 0);
  out[p] = solar_point<Out>(la, lo, nnodes, [&](unsigned k, int j) -> double { return nodes[(size_t)k * kSolarRecord + j]; });
}

template <class T>
static int solar_operand(const char* name, const ekm_operand* op, size_t n, SolarOperand<T>* o, bool* small) {
  if (!op || !op->data) return set_error(EKM_ERR_ARG, "solar: %s: null pointer", name);
  if (reinterpret_cast<uintptr_t>(op->data) % sizeof(T))
    return set_error(EKM_ERR_ARG, "solar: %s is not aligned to its element size (%d B)", name, (int)sizeof(T));
  o->data = static_cast<const T*>(op->data);
  o->mode = op->mode;
  o->len = 1;
  o->inner = 1;
  switch (op->mode) {
    case EKM_FIELD:
    case EKM_SCALAR:
      break;
    case EKM_LEVEL_MAJOR:
      if (op->len == 0 || op->inner == 0 || op->len < (n + op->inner - 1) / op->inner)
        return set_error(EKM_ERR_ARG, "solar: %s: len * inner = %llu * %llu does not cover n = %llu", name,
                         (unsigned long long)op->len, (unsigned long long)op->inner, (unsigned long long)n);
      o->len = op->len;
      o->inner = op->inner;
      break;
    case EKM_LEVEL_MINOR:
      if (op->len == 0) return set_error(EKM_ERR_ARG, "solar: %s: an empty vector", name);
      o->len = op->len;
      break;
    default:
      return set_error(EKM_ERR_ARG, "solar: %s: mode %d is not EKM_FIELD, EKM_SCALAR, EKM_LEVEL_MAJOR or EKM_LEVEL_MINOR", name,
                       op->mode);
  }
  if (o->len > 0xffffffffull || o->inner > 0xffffffffull) *small = false;
  return EKM_OK;
}

template <class T, class Out>
static int launch_solar(int dev, void* stream, const ekm_operand* lat, const ekm_operand* lon, const double* nodes,
                        uint32_t nnodes, Out* out, size_t n) {
  if (n == 0) return EKM_OK;
  if (nnodes > 0 && (!nodes || reinterpret_cast<uintptr_t>(nodes) % sizeof(double)))
    return set_error(EKM_ERR_ARG, "solar: the node records are null or not 8-B aligned");
  if (!out || reinterpret_cast<uintptr_t>(out) % sizeof(Out))
    return set_error(EKM_ERR_ARG, "solar: out is null or not aligned to its element size (%d B)", (int)sizeof(Out));
  bool small = (unsigned long long)n <= 0x100000000ull;  // 32-bit index arithmetic for the vector operands
  SolarOperand<T> la, lo;
  int rc = solar_operand<T>("latitudes", lat, n, &la, &small);
  if (rc != EKM_OK) return rc;
  rc = solar_operand<T>("longitudes", lon, n, &lo, &small);
  if (rc != EKM_OK) return rc;
  const unsigned long long g = ((unsigned long long)n + kSolarThreads - 1) / kSolarThreads;
  if (g > 0x7fffffffull) return set_error(EKM_ERR_ARG, "solar: too many points");
  rc = use_device(dev);
  if (rc != EKM_OK) return rc;
  hipLaunchKernelGGL((solar_points<T, Out>), dim3((unsigned)g), dim3(kSolarThreads), 0, static_cast<hipStream_t>(stream), la, lo,
                     nodes, nnodes, (unsigned long long)n, small ? 1 : 0, out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(EKM_ERR_HIP, "solar launch: %s", hipGetErrorString(e));
  return EKM_OK;
}

}  // namespace ekm

extern "C" {

int ekm_solar_f32(int dev, void* stream, const ekm_operand* lat, const ekm_operand* lon, const double* nodes, uint32_t nnodes,
                  float* out, size_t n) {
  return ekm::launch_solar<float, float>(dev, stream, lat, lon, nodes, nnodes, out, n);
}
int ekm_solar_f64(int dev, void* stream, const ekm_operand* lat, const ekm_operand* lon, const double* nodes, uint32_t nnodes,
                  double* out, size_t n) {
  return ekm::launch_solar<double, double>(dev, stream, lat, lon, nodes, nnodes, out, n);
}
int ekm_solar_f32_f64(int dev, void* stream, const ekm_operand* lat, const ekm_operand* lon, const double* nodes,
                      uint32_t nnodes, double* out, size_t n) {
  return ekm::launch_solar<float, double>(dev, stream, lat, lon, nodes, nnodes, out, n);
}

}  // extern "C"
