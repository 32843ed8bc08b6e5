// hpc_host.cpp — the part of "homopolymer compression" (include/mhap_hip.h) that needs no GPU: one record expanded through two explicit
// maps.  The rule is hpc_common.hpp's, the one expand_kernel (hpc_kernels.hip) runs per lane.
#include "hpc_common.hpp"

extern "C" int mhap_hpc_expand_record(const mhap_record* in, const int32_t* start_from, int32_t clen_from, const int32_t* start_to,
                                      int32_t clen_to, mhap_record* out) {
  if (!in || !start_from || !start_to || !out || clen_from < 0 || clen_to < 0) return -1;
  const mhap::HpcEnds e = mhap::hpc_expand(in->a1, in->a2, in->b1, in->b2, start_from, clen_from, start_to, clen_to);
  *out = *in;
  out->a1 = e.a1; out->a2 = e.a2; out->alen = e.alen;
  out->b1 = e.b1; out->b2 = e.b2; out->blen = e.blen;
  return 0;
}
