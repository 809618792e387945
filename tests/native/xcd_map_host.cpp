// Host build of csrc/td7_xcd_map.h for tests/test_xcd_map_host.py.
#include "td7_xcd_map.h"

extern "C" {
int xm_num_xcd() { return EXO_NUM_XCD; }
// out[b] = xcd_contiguous(b, total) for b in 0 .. total-1
void xm_map(int total, int *out) {
    for (int b = 0; b < total; ++b) out[b] = xcd_contiguous(b, total);
}
}
