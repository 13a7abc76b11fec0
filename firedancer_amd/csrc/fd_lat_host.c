/* Host build of the device half-size-scalar reductions (fd_gpu_lattice.h),
   for tests/test_lattice.py and tests/test_lattice_skew.py: the same source
   the hash kernel inlines. */
#include "fd_gpu_lattice.h"

int
fd_lat_halfsize_host( uint32_t c0[ 5 ], uint32_t c1m[ 5 ], int * c1neg, uint32_t const k[ 8 ] ) {
  return fd_lat_halfsize( c0, c1m, c1neg, k );
}

int
fd_lat_skew_host( uint32_t c0[ 7 ], uint32_t c1m[ 5 ], int * c1neg, int * nwin, uint32_t const k[ 8 ] ) {
  return fd_lat_skew( c0, c1m, c1neg, nwin, k );
}

/* n scalars at once: k[8 n] -> c0[7 n], c1m[5 n], neg[n], nwin[n], ok[n] */
void
fd_lat_skew_host_many( unsigned long n, uint32_t const * k, uint32_t * c0, uint32_t * c1m, int * neg, int * nwin,
                       int * ok ) {
  for( unsigned long i=0UL; i<n; i++ ) {
    neg[i] = 0; nwin[i] = 0;
    ok[i] = fd_lat_skew( c0 + 7UL*i, c1m + 5UL*i, neg + i, nwin + i, k + 8UL*i );
  }
}

/* the fixed-base walk's digits of k (tests/test_fb_recode.py) */
int
fd_fb_recode_host( signed char d[ 32 ], uint32_t const k[ 8 ] ) {
  return fd_fb_recode( d, k );
}
