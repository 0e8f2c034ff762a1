// Which reduction kernel open_pcc_metric_amd/csrc/pccm_reduce_shape.h picks, over the whole domain of a job's layout fields:
// one line per job, compared by tests/test_reduce_shape_host.py with tests/golden/reduce_dispatch.txt.  Host code only; built
// with the host sanitizers and run as a process of its own.
#include <cstdio>

#include "pccm_reduce_shape.h"

int main()
{
    using namespace pccm;
    const int strides[3] = {1, 2, 4};
    int jobs = 0;
    for (int stride : strides)
        for (int ncols = 1; ncols <= 2; ++ncols)
            for (int bits = 0; bits < 16; ++bits)
                for (int defer = 0; defer <= 5; ++defer) {
                    UnitJob J = {};
                    J.stride = stride;
                    J.ncols = ncols;
                    J.c[0].off = bits >> 3 & 1;
                    J.c[0].square = bits >> 2 & 1;
                    J.c[1].off = bits >> 1 & 1;
                    J.c[1].square = bits & 1;
                    J.defer = defer;
                    printf("stride %d ncols %d c0 off %d square %d c1 off %d square %d defer %d: ", stride, ncols, J.c[0].off, J.c[0].square,
                           J.c[1].off, J.c[1].square, defer);
                    const int row = lean_index(reduce_shape(J));
                    if (row < 0) printf("general\n");
                    else printf("k_unit_lean<%d, %d, %d>\n", kLeanShapes[row].stride, kLeanShapes[row].cfg, kLeanShapes[row].defer);
                    ++jobs;
                }
    return jobs == 576 ? 0 : 1;
}
