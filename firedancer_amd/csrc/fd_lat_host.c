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

/* the two fixed-base walks' schedules (tests/test_fb_full_schedule.py): out[0] = additions of old step r, then per
   addition (is_base, digit, table); likewise the body without doublings */
int
fd_fb_old_sched_host( int r, int * out ) {
  int na = fd_fb_old_adds( r );
  for( int i=0; i<na; i++ ) { out[3*i] = fd_fb_old_is_base( i ); out[3*i+1] = fd_fb_old_digit( r, i ); out[3*i+2] = fd_fb_old_table( i ); }
  return na;
}

int
fd_fb_full_sched_host( int * out ) {
  for( int i=0; i<FD_FB_FULL_ADDS; i++ ) { out[3*i] = fd_fb_full_is_base( i ); out[3*i+1] = fd_fb_full_digit( i ); out[3*i+2] = fd_fb_full_table( i ); }
  return FD_FB_FULL_ADDS;
}

int
fd_fb_entry_host( int d ) { return fd_fb_entry( d ); }

int
fd_fb_tables_host( int * nt, int * nb ) { *nt = FD_FB_NT; *nb = FD_FB_NB; return 0; }
