// The split-bf16 product module (split3.hip): the fp32-grade products of loss.hip (K9's similarity) and classifier.hip (the linear-probe head).
//   v = hi + lo (bf16 each);  <x, y> ~ hi·hi + hi·lo + lo·hi  as ONE NT GEMM with K = 3D over [hi|hi|lo] (x side) and [hi|lo|hi] (y side).
// Kernels, segment orders, padding and GEMM calls live in split3.hip, once in the code object; declarations only here (not C-ABI symbols).
#pragma once
#include "host_util.h"

namespace clibd {

enum Split3Side { SPLIT3_Y = 0, SPLIT3_X = 1 };   // [hi|lo|hi] / [hi|hi|lo]

// The operand images of the products of x [M,D] and y [N,D], carved in this order.
struct Split3Ws {
    unsigned short *x3, *y3;   // [M,3D] = [hi|hi|lo],  [pad16(N),3D] = [hi|lo|hi] (rows N.. zero)
    unsigned short *G, *GT;    // the coefficients g [M,N]: [M,3Np] = [hi|hi|lo],  [N,3Mp] = [hi^T|lo^T|hi^T]      (Np = pad64(N), Mp = pad64(M))
    unsigned short *xT, *yT;   // [D,3Mp] = [hi^T|hi^T|lo^T],  [D,3Np] = [hi^T|lo^T|hi^T]
    void carve(Carver& c, int M, int N, int D);
};

// out[r, 0:Cp | Cp:2Cp | 2Cp:3Cp] = the side's image of in[r, 0:C] (row stride ld_in), segments zero padded to Cp columns; `grid` workgroups
// of a grid-stride loop; `what` names the launch in an error.
int split3_image(const float* in, int ld_in, int R, int C, int Cp, Split3Side side, unsigned short* out, unsigned grid, const char* what,
                 hipStream_t st);

// out[M, pad16(N)] (ld = pad16(N), columns N.. are those of zero rows) = x · yᵀ (+ bias16[pad16(N)] if given).  Splits x into ws.x3 and y
// into ws.y3 with grid_x / grid_y workgroups and zeroes the padded rows of ws.y3.  `op` names the entry point in the memset's error,
// `what` the split launches.
int split3_forward(const float* x, const float* y, int M, int N, int D, const float* bias16, float* out, const Split3Ws& ws, unsigned grid_x,
                   unsigned grid_y, const char* op, const char* what, hipStream_t st);

// dx[M,D] (+)= g · y from ws.G (the caller writes the [hi|hi|lo] image of g, e.g. with split3_image) and ws.y3; uses ws.yT
int split3_grad_left(float* dx, bool accumulate, int M, int N, int D, const Split3Ws& ws, hipStream_t st);
// dy[N,D] (+)= gᵀ · x from ws.G and ws.x3; uses ws.GT and ws.xT
int split3_grad_right(float* dy, bool accumulate, int M, int N, int D, const Split3Ws& ws, hipStream_t st);

}  // namespace clibd
