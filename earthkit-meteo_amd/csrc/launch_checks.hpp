// The argument checks every launcher outside the map kernels makes before it launches, and the check after it: host
// side only.  Each returns EKM_OK or the code set_error recorded.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>

#include "../../include/ekm_thermo.h"
#include "map_kernel.hpp"
#include "point_operand.hpp"

namespace ekm {

inline bool misaligned(const void* ptr, size_t elem) { return reinterpret_cast<uintptr_t>(ptr) % elem != 0; }

// Pointers that may be null but must be aligned to their element (`elem` bytes) when given
inline int check_aligned_if_given(const char* what, size_t elem, std::initializer_list<const void*> ptrs) {
  for (const void* ptr : ptrs)
    if (ptr && misaligned(ptr, elem))
      return set_error(EKM_ERR_ARG, "%s: a pointer is not aligned to its element size (%d B)", what, (int)elem);
  return EKM_OK;
}

// Required pointers: none null, each aligned to its element
inline int check_pointers(const char* what, size_t elem, std::initializer_list<const void*> ptrs) {
  for (const void* ptr : ptrs)
    if (!ptr) return set_error(EKM_ERR_ARG, "%s: null pointer", what);
  return check_aligned_if_given(what, elem, ptrs);
}

// ceil(items / per_block) workgroups along x; a grid dimension is held to 31 bits
inline int launch_grid(const char* what, unsigned long long items, unsigned per_block, unsigned* grid) {
  const unsigned long long g = items / per_block + (items % per_block != 0);
  if (g > 0x7fffffffull) return set_error(EKM_ERR_ARG, "%s: too many points for one launch", what);
  *grid = (unsigned)g;
  return EKM_OK;
}

static_assert(EKM_SCALAR == 1 && EKM_LEVEL_MAJOR == 2 && EKM_LEVEL_MINOR == 3, "point_operand.hpp::point_fetch and the header disagree");

// Operand `name` of `what` for n points.  *small: no vector too long for 32-bit indices; *fields: every operand a field.
template <class T>
inline int check_point_operand(const char* what, const char* name, const ekm_operand* op, size_t n, PointOperand<T>* o,
                               bool* small, bool* fields = nullptr) {
  if (!op || !op->data) return set_error(EKM_ERR_ARG, "%s: %s: null pointer", what, name);
  if (misaligned(op->data, sizeof(T)))
    return set_error(EKM_ERR_ARG, "%s: %s is not aligned to its element size (%d B)", what, name, (int)sizeof(T));
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
        return set_error(EKM_ERR_ARG, "%s: %s: len * inner = %llu * %llu does not cover n = %llu", what, name,
                         (unsigned long long)op->len, (unsigned long long)op->inner, (unsigned long long)n);
      o->len = op->len;
      o->inner = op->inner;
      break;
    case EKM_LEVEL_MINOR:
      if (op->len == 0) return set_error(EKM_ERR_ARG, "%s: %s: an empty vector", what, name);
      o->len = op->len;
      break;
    default:
      return set_error(EKM_ERR_ARG, "%s: %s: mode %d is not EKM_FIELD, EKM_SCALAR, EKM_LEVEL_MAJOR or EKM_LEVEL_MINOR", what, name,
                       op->mode);
  }
  if (fields && op->mode != EKM_FIELD) *fields = false;
  if (o->len > 0xffffffffull || o->inner > 0xffffffffull) *small = false;
  return EKM_OK;
}

inline int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(EKM_ERR_HIP, "%s launch: %s", what, hipGetErrorString(e));
  return EKM_OK;
}

}  // namespace ekm
