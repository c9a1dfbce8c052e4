// An operand of a one-lane-per-point kernel (solar.hip, wind.hip) and of the host test twin, indexed where it lies and
// never expanded.  launch_checks.hpp::check_point_operand fills one from an ekm_operand.
#pragma once

#include "thermo_math.hpp"

namespace ekm {

// Element of an operand for flat point p: a full field, one value, a vector along the leading axes (p / inner) or along
// the trailing axes (p % len).  The modes are EKM_FIELD .. EKM_LEVEL_MINOR of include/ekm_thermo.h.
template <class T>
struct PointOperand {
  const T* data;
  int mode;
  unsigned long long len, inner;
};

template <class T>
EKM_HD double point_fetch(const PointOperand<T>& o, unsigned long long p, bool small) {
  unsigned long long i = p;
  if (o.mode == 1) {
    i = 0;
  } else if (o.mode == 2) {
    i = small ? (unsigned long long)((unsigned)p / (unsigned)o.inner) : p / o.inner;
    if (i >= o.len) i = o.len - 1;
  } else if (o.mode == 3) {
    i = small ? (unsigned long long)((unsigned)p % (unsigned)o.len) : p % o.len;
  }
  return (double)o.data[i];
}

}  // namespace ekm
