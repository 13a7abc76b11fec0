/* Stand-alone check of fd_pin_list.h, the host side of fdgpu_ed25519_set_pinned_keys' key list: the cap and the
   de-duplication, against a quadratic reference.  tests/test_pin_list.py compiles and runs it; built with
   -fsanitize=address,undefined it also checks the table and the output arrays for overruns.  Exit status 0 and
   "ok" on success. */

#include <stdio.h>
#include <stdlib.h>
#include "fd_pin_list.h"

static unsigned long rng_state = 0x9e3779b97f4a7c15UL;
static unsigned long rng( void ) {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}

static int check( unsigned long n, unsigned long pool ) {
  /* exact-size allocations, so that a sanitizer sees an index one past the end */
  unsigned char * keys     = malloc( n ? 32UL * n : 1UL );
  unsigned int *  slot_of  = malloc( ( n ? n : 1UL ) * sizeof(unsigned int) );
  unsigned int *  first_of = malloc( ( n ? n : 1UL ) * sizeof(unsigned int) );
  unsigned int *  work     = malloc( fd_pin_list_work( n ) * sizeof(unsigned int) );
  if( !keys || !slot_of || !first_of || !work ) return 1;
  for( unsigned long i=0UL; i<n; i++ ) {
    /* keys from a small pool (pool = 0: all distinct), equal in all bytes but a few, so that the probes collide */
    unsigned long id = pool ? rng() % pool : i;
    memset( keys + 32UL*i, 0xa5, 32UL );
    keys[ 32UL*i + 31UL ] = (unsigned char)id; keys[ 32UL*i ] = (unsigned char)( id >> 8 ); keys[ 32UL*i + 7UL ] = (unsigned char)( id >> 16 );
  }
  unsigned long m = fd_pin_list_dedup( keys, n, slot_of, first_of, work );
  int bad = 0;
  unsigned long want_m = 0UL;
  for( unsigned long i=0UL; i<n; i++ ) {
    unsigned long f = i;
    for( unsigned long j=0UL; j<i; j++ ) if( !memcmp( keys + 32UL*j, keys + 32UL*i, 32UL ) ) { f = j; break; }
    if( f == i ) {                   /* a first appearance: the next number */
      if( slot_of[i] != want_m || first_of[want_m] != i ) bad = 1;
      want_m++;
    } else if( slot_of[i] != slot_of[f] ) bad = 1;
  }
  if( m != want_m ) bad = 1;
  if( bad ) fprintf( stderr, "fd_pin_list_dedup wrong: n %lu pool %lu m %lu want %lu\n", n, pool, m, want_m );
  free( keys ); free( slot_of ); free( first_of ); free( work );
  return bad;
}

int main( void ) {
  int bad = 0;
  unsigned long const ns[] = { 0UL, 1UL, 2UL, 3UL, 4UL, 5UL, 24UL, 25UL, 767UL, 768UL, 3072UL };
  for( unsigned long k=0UL; k<sizeof(ns)/sizeof(ns[0]); k++ ) {
    bad |= check( ns[k], 0UL );      /* all distinct */
    bad |= check( ns[k], 1UL );      /* all the same */
    bad |= check( ns[k], 7UL );
    bad |= check( ns[k], ns[k] / 2UL + 1UL );
  }
  /* the cap: three quarters of the slots, rounded up; the work table at least twice the list, a power of two */
  if( fd_pin_list_cap( 0UL ) != 0UL || fd_pin_list_cap( 1UL ) != 1UL || fd_pin_list_cap( 3UL ) != 3UL || fd_pin_list_cap( 8UL ) != 6UL
      || fd_pin_list_cap( 32UL ) != 24UL || fd_pin_list_cap( 1024UL ) != 768UL || fd_pin_list_cap( 4096UL ) != 3072UL ) {
    fprintf( stderr, "fd_pin_list_cap wrong\n" ); bad = 1;
  }
  for( unsigned long n=0UL; n<5000UL; n++ ) {
    unsigned long w = fd_pin_list_work( n );
    if( w < 2UL*n || w < 4UL || ( w & ( w - 1UL ) ) ) { fprintf( stderr, "fd_pin_list_work wrong at %lu\n", n ); bad = 1; break; }
  }
  if( !bad ) puts( "ok" );
  return bad;
}
