// What conv2d_gen.hip and conv2d.hip share: the geometry of a 2-D convolution between a small and a big map (conv2d_gen.hip says
// how the two are tied), and the launchers of the (3,9) kernels that the generic entry points try first.
#pragma once
#include "common.h"

struct CGen {
  int B, Cs, Hs, Ws, Cb, Hb, Wb, kh, kw, sh, sw, ph, pw;
  int64_t ssb, ssy, ssx, ssc;   // strides of the small map
  int64_t gsb, gsy, gsx, gsc;   // strides of the big map
};

// conv2d.hip, called by maavss_conv2d_gen_{small,big,wgrad,wgrad_ws_bytes} for a call without bias.  k39_small / k39_big launch
// and return true exactly when the call is one their kernel was written for, else they do nothing; k39_wgrad_nchunk is the row
// kernel's number of partial sums for such a call and 0 for any other; k39_wgrad (ws: nchunk * Cs*Cb*27 floats) takes that number.
bool conv2d_k39_small(const float* big, const float* w, float* small, const CGen& g, hipStream_t st);
bool conv2d_k39_big(const float* small, const float* w, float* big, const CGen& g, hipStream_t st);
int conv2d_k39_wgrad_nchunk(const CGen& g);
void conv2d_k39_wgrad(const float* small, const float* big, float* dw, float* ws, const CGen& g, int nchunk, int beta, hipStream_t st);
