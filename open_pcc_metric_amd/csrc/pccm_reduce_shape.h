// Which reduction kernel takes a job: the shape of a UnitJob as far as a kernel compiled for one shape cares, and the shapes
// that have such a kernel (k_unit_lean; kLeanKernels in pccm_point.hip holds the kernel of each, checked against this list row
// by row; DESIGN.md, K5, has it as a table).  Host-only: no HIP call, no allocation.
#pragma once
#include "pccm_internal.h"

namespace pccm {

// stride: doubles per record (1: a plain column).  cfg: which fields feed the columns -- 0: two columns {field 0, field 1
// squared} (D1 + D2 of a direction in one pass over its records), 1: field 0, 2: field 1 squared, 3: field 1 (the signed
// projection), -1: anything else -- a job with a mapped column (UnitCol::map) among them: only the general kernel maps.
// defer: UnitJob::defer (records of layout 1, stride 2).
struct ReduceShape {
    int stride, cfg, defer;
};
constexpr bool operator==(const ReduceShape &a, const ReduceShape &b) { return a.stride == b.stride && a.cfg == b.cfg && a.defer == b.defer; }

inline ReduceShape reduce_shape(const UnitJob &J)
{
    int cfg = -1;
    if (J.stride == 1) cfg = (J.ncols == 1 && J.c[0].off == 0 && !J.c[0].square) ? 1 : -1;
    else if (J.ncols == 2) cfg = (J.c[0].off == 0 && !J.c[0].square && J.c[1].off == 1 && J.c[1].square) ? 0 : -1;
    else if (J.c[0].off == 0) cfg = J.c[0].square ? -1 : 1;
    else cfg = J.c[0].square ? 2 : 3;
    if (J.c[0].map || (J.ncols == 2 && J.c[1].map)) cfg = -1;
    if (cfg < 0 || (J.stride != 1 && J.stride != 2 && J.stride != 4) || (J.defer && J.stride != 2)) return {0, -1, 0};
    return {J.stride, cfg, J.defer};
}

// The shapes with a kernel of their own.  cfg 3 is not among them: a signed projection column holds -0.0 beside 0.0, which only
// fmin / fmax order, and the lean kernels use the raw instructions.
constexpr ReduceShape kLeanShapes[] = {
    {1, 1, 0}, {2, 0, 0}, {2, 1, 0}, {2, 2, 0}, {4, 0, 0}, {4, 1, 0}, {4, 2, 0}, {2, 0, 1}, {2, 1, 1}, {2, 2, 1},
    {2, 0, 2}, {2, 1, 2}, {2, 2, 2}, {2, 1, 3}, {2, 0, 4}, {2, 2, 4}, {2, 0, 5}, {2, 2, 5},
};
constexpr int kLeanCount = (int)(sizeof(kLeanShapes) / sizeof(kLeanShapes[0]));

constexpr int lean_index(const ReduceShape &s)          // row of kLeanShapes, or -1: the general kernel
{
    for (int i = 0; i < kLeanCount; ++i)
        if (kLeanShapes[i] == s) return i;
    return -1;
}

}  // namespace pccm
