/* Stand-alone check of fd_sig_desc.h, the validity test, packed size and placement of per-signature descriptors
   (fdgpu_sig_desc_t): the edges of every range against the arena's end, offsets near 2^32, the longest message, the
   sizes of tests/test_gpu_sigs.py's message list, and the placement -- offsets, flags and the records that fit --
   against a reference written another way, at capacities that end exactly on, one byte before and one byte after
   a record.  tests/test_sig_desc.py compiles and runs it; built with -fsanitize=address,undefined it also checks
   the output arrays for overruns.  Exit status 0 and "ok" on success. */

#include <stdio.h>
#include <stdlib.h>
#include "fd_sig_desc.h"

static int fails;
#define CHECK( c ) do { if( !(c) ) { fprintf( stderr, "line %d: %s\n", __LINE__, #c ); fails++; } } while(0)

static unsigned long rng_state = 0x9e3779b97f4a7c15UL;
static unsigned long rng( void ) {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}

static unsigned int size_of( unsigned int s, unsigned int p, unsigned int m, unsigned int z, unsigned long a, int * bad ) {
  return fd_sig_desc_size( s, p, m, z, a, bad );
}

static void check_edges( void ) {
  unsigned long const A = 4096UL;
  int bad;
  /* each range ending exactly at the arena's end is good, one byte further is bad */
  CHECK( !fd_sig_desc_bad( (unsigned)A - 64U, 0U, 0U, 0U, A ) );
  CHECK(  fd_sig_desc_bad( (unsigned)A - 63U, 0U, 0U, 0U, A ) );
  CHECK( !fd_sig_desc_bad( 0U, (unsigned)A - 32U, 0U, 0U, A ) );
  CHECK(  fd_sig_desc_bad( 0U, (unsigned)A - 31U, 0U, 0U, A ) );
  CHECK( !fd_sig_desc_bad( 0U, 64U, (unsigned)A - 100U, 100U, A ) );
  CHECK(  fd_sig_desc_bad( 0U, 64U, (unsigned)A - 100U, 101U, A ) );
  CHECK(  fd_sig_desc_bad( 0U, 64U, (unsigned)A - 99U, 100U, A ) );
  /* an empty message may sit at the very end, not past it */
  CHECK( !fd_sig_desc_bad( 0U, 64U, (unsigned)A, 0U, A ) );
  CHECK(  fd_sig_desc_bad( 0U, 64U, (unsigned)A + 1U, 0U, A ) );
  /* offsets near 2^32: no wrap, also under the largest arena an offset can name */
  CHECK(  fd_sig_desc_bad( 0xFFFFFFF0U, 0U, 0U, 0U, A ) );
  CHECK(  fd_sig_desc_bad( 0U, 0xFFFFFFF0U, 0U, 0U, A ) );
  CHECK(  fd_sig_desc_bad( 0U, 64U, 0xFFFFFFFFU, 2U, A ) );
  CHECK(  fd_sig_desc_bad( 0xFFFFFFF0U, 0U, 0U, 0U, 0xFFFFFFFFUL ) );
  CHECK(  fd_sig_desc_bad( 0U, 64U, 0xFFFFFFFFU, 2U, 0xFFFFFFFFUL ) );
  CHECK( !fd_sig_desc_bad( 0xFFFFFFF0U, 0U, 0U, 0U, 0x100000030UL ) );
  CHECK( !fd_sig_desc_bad( 0U, 64U, 0xFFFFFFFFU, 2U, 0x100000001UL ) );
  /* the longest message */
  CHECK( !fd_sig_desc_bad( 0U, 64U, 96U, 65439U, 1UL << 20 ) );
  CHECK(  fd_sig_desc_bad( 0U, 64U, 96U, 65440U, 1UL << 20 ) );
  CHECK(  fd_sig_desc_bad( 0U, 64U, 96U, 0xFFFFFFFFU, 1UL << 20 ) );
  CHECK(  fd_sig_desc_bad( 0U, 64U, 96U, 0xFFFFFFFFU, 0x200000000UL ) );
  CHECK( size_of( 0U, 64U, 96U, 65439U, 1UL << 20, &bad ) == 65536U && !bad );
  CHECK( size_of( 0U, 64U, 96U, 65440U, 1UL << 20, &bad ) == 96U && bad == 1 );
  /* an empty arena holds nothing, not even an empty message's signature */
  CHECK( fd_sig_desc_bad( 0U, 0U, 0U, 0U, 0UL ) );
  /* sizes: 96 + msg_sz rounded up to 8 */
  static unsigned int const szs[] = { 0U, 1U, 3U, 4U, 5U, 7U, 8U, 9U, 15U, 16U, 17U, 31U, 32U, 33U, 63U, 64U, 65U, 127U, 128U,
                                      129U, 255U, 256U, 257U, 1167U, 1232U, 4095U, 4096U, 65439U };
  for( unsigned long k=0UL; k<sizeof(szs)/sizeof(szs[0]); k++ ) {
    unsigned int z = size_of( 0U, 64U, 96U, szs[k], 1UL << 20, &bad );
    CHECK( !bad && !( z & 7U ) && z >= 96U + szs[k] && z < 96U + szs[k] + 8U );
  }
}

/* the placement of cnt random descriptors (a tenth of them bad) under capacity cap, against sums recomputed from
   scratch for every record */
static void check_place( unsigned long cnt, unsigned long cap_sel ) {
  unsigned long const A = 1UL << 16;
  unsigned int *  d    = malloc( ( cnt ? cnt : 1UL ) * 4UL * sizeof(unsigned int) );
  unsigned long * off  = malloc( ( cnt ? cnt : 1UL ) * sizeof(unsigned long) );
  unsigned char * flag = malloc( cnt ? cnt : 1UL );
  if( !d || !off || !flag ) { fails++; return; }
  for( unsigned long i=0UL; i<cnt; i++ ) {
    unsigned int z = (unsigned int)( rng() % 1233UL );
    d[4UL*i] = (unsigned int)( rng() % ( A - 64UL ) ); d[4UL*i+1UL] = (unsigned int)( rng() % ( A - 32UL ) );
    d[4UL*i+2UL] = (unsigned int)( rng() % ( A - z ) ); d[4UL*i+3UL] = z;
    if( rng() % 10UL == 0UL ) d[4UL*i + rng() % 3UL] = (unsigned int)A;      /* one byte past, whatever the field */
  }
  /* the total, and the end of a record in the middle, for the capacities */
  unsigned long total = 0UL, mid_end = 0UL;
  for( unsigned long i=0UL; i<cnt; i++ ) {
    int bad;
    total += size_of( d[4UL*i], d[4UL*i+1UL], d[4UL*i+2UL], d[4UL*i+3UL], A, &bad );
    if( i == cnt / 2UL ) mid_end = total;
  }
  unsigned long cap = cap_sel == 0UL ? total : cap_sel == 1UL ? total - ( total ? 1UL : 0UL ) : cap_sel == 2UL ? mid_end
                    : cap_sel == 3UL ? mid_end + 1UL : cap_sel == 4UL ? ( mid_end ? mid_end - 1UL : 0UL ) : 0UL;
  unsigned long fit = fd_sig_desc_place( d, cnt, A, cap, off, flag );
  unsigned long want_fit = cnt;
  int seen_over = 0;
  for( unsigned long i=0UL; i<cnt; i++ ) {
    unsigned long at = 0UL;
    for( unsigned long j=0UL; j<i; j++ ) {
      int b = d[4UL*j] > A - 64UL || d[4UL*j+1UL] > A - 32UL || (unsigned long)d[4UL*j+2UL] + d[4UL*j+3UL] > A;
      at += b ? 96UL : ( 96UL + d[4UL*j+3UL] + 7UL ) / 8UL * 8UL;
    }
    int b = d[4UL*i] > A - 64UL || d[4UL*i+1UL] > A - 32UL || (unsigned long)d[4UL*i+2UL] + d[4UL*i+3UL] > A;
    unsigned long end = at + ( b ? 96UL : ( 96UL + d[4UL*i+3UL] + 7UL ) / 8UL * 8UL );
    int over = end > cap;
    CHECK( off[i] == at );
    CHECK( flag[i] == ( ( b ? FD_SIG_DESC_BAD : 0 ) | ( over ? FD_SIG_DESC_OVER : 0 ) ) );
    CHECK( !seen_over || over );               /* once past the capacity, every later record is */
    if( over && !seen_over ) { seen_over = 1; want_fit = i; }
  }
  CHECK( fit == want_fit );
  if( cap_sel == 0UL ) CHECK( fit == cnt );
  if( cap_sel == 2UL && cnt ) CHECK( fit == cnt / 2UL + 1UL );
  if( cap_sel == 4UL && cnt ) CHECK( fit == cnt / 2UL );
  free( d ); free( off ); free( flag );
}

int main( void ) {
  check_edges();
  unsigned long const ns[] = { 0UL, 1UL, 2UL, 63UL, 64UL, 65UL, 255UL, 256UL, 257UL, 700UL };
  for( unsigned long k=0UL; k<sizeof(ns)/sizeof(ns[0]); k++ )
    for( unsigned long c=0UL; c<6UL; c++ ) check_place( ns[k], c );
  if( !fails ) puts( "ok" );
  return fails ? 1 : 0;
}
