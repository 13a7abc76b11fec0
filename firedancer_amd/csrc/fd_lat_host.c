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

/* the wide walk's schedule and split (tests/test_fb_wide_schedule.py): per addition (is_base, span, digit, table);
   a wave's additions; a span's digit; the geometry (W0, W2, entries per span, wcap) and a table's size and offset */
int
fd_fb_wide_sched_host( int * out ) {
  for( int i=0; i<FD_FB_WIDE_ADDS; i++ ) {
    out[4*i] = fd_fb_wide_is_base( i ); out[4*i+1] = fd_fb_wide_span( i ); out[4*i+2] = fd_fb_wide_digit( i ); out[4*i+3] = fd_fb_wide_table( i );
  }
  return FD_FB_WIDE_ADDS;
}

int
fd_fb_wave_adds_host( int all_wide ) { return fd_fb_wave_adds( all_wide ); }

int
fd_fb_wide_split_host( int a0, int a1, int a2, int a3, int r ) { return fd_fb_wide_split( a0, a1, a2, a3, r ); }

int
fd_fb_wide_geom_host( int * w0, int * w2, int * we, int * wcap ) { *w0 = FD_FB_W0; *w2 = FD_FB_W2; *we = FD_FB_WE; *wcap = FD_FB_WCAP; return 0; }

int
fd_fb_wide_entries_host( int r ) { return fd_fb_wide_entries( r ); }

int
fd_fb_wide_off_host( int t, int r ) { return fd_fb_wide_off( t, r ); }
