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
#include "launch_checks.hpp"
#include "map_kernel.hpp"
#include "solar_point.hpp"

namespace ekm {

constexpr int kSolarThreads = 256;

template <class T, class Out>
__global__ __launch_bounds__(kSolarThreads) void solar_points(const PointOperand<T> lat, const PointOperand<T> lon,
                                                              const double* __restrict__ nodes, unsigned nnodes,
                                                              unsigned long long n, int small, Out* __restrict__ out) {
  const unsigned long long p = (unsigned long long)blockIdx.x * kSolarThreads + threadIdx.x;
  if (p >= n) return;
  const double la = point_fetch<T>(lat, p, small != 0), lo = point_fetch<T>(lon, p, small != 0);
  out[p] = solar_point<Out>(la, lo, nnodes, [&](unsigned k, int j) -> double { return nodes[(size_t)k * kSolarRecord + j]; });
}

template <class T, class Out>
static int launch_solar(int dev, void* stream, const ekm_operand* lat, const ekm_operand* lon, const double* nodes,
                        uint32_t nnodes, Out* out, size_t n) {
  if (n == 0) return EKM_OK;
  int rc = nnodes > 0 ? check_pointers("solar", sizeof(double), {nodes}) : EKM_OK;
  if (rc == EKM_OK) rc = check_pointers("solar", sizeof(Out), {out});
  if (rc != EKM_OK) return rc;
  bool small = (unsigned long long)n <= 0x100000000ull;  // 32-bit index arithmetic for the vector operands
  PointOperand<T> la, lo;
  if ((rc = check_point_operand<T>("solar", "latitudes", lat, n, &la, &small)) != EKM_OK) return rc;
  if ((rc = check_point_operand<T>("solar", "longitudes", lon, n, &lo, &small)) != EKM_OK) return rc;
  unsigned grid;
  if ((rc = launch_grid("solar", n, kSolarThreads, &grid)) != EKM_OK) return rc;
  if ((rc = use_device(dev)) != EKM_OK) return rc;
  hipLaunchKernelGGL((solar_points<T, Out>), dim3(grid), dim3(kSolarThreads), 0, static_cast<hipStream_t>(stream), la, lo,
                     nodes, nnodes, (unsigned long long)n, small ? 1 : 0, out);
  return launched("solar");
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
