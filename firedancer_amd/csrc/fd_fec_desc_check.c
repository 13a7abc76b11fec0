/* Stand-alone check of fd_fec_desc.h, the shape of a FEC set's Merkle tree and the rules that give a set
   (fdgpu_fec_desc_t) its code before any hashing: the depth, the layer sizes and every leaf's proof node at every
   layer for every n <= 256 against a tree laid out by a plain loop; every descriptor, range and member rule one
   value on each side of its edge.  firedancer_amd/build.py builds it and tests/test_fec_desc.py runs it.  Exit
   status 0 and "ok" on success. */

#include <stdio.h>
#include <string.h>
#include "fd_fec_desc.h"

static int fails;
#define CHECK( c ) do { if( !(c) ) { fprintf( stderr, "line %d: %s\n", __LINE__, #c ); fails++; } } while(0)

/* ---- the tree's shape ------------------------------------------------------------------------------------- */

/* The tree of n leaves by the plain rule: build layer after layer until one node is left, pairing node 2j with
   node 2j + 1 or, at the end of an odd layer, with itself.  who[l][j] is the partner that node j of layer l is
   merged with (its proof node). */
static unsigned int who[ 10 ][ 256 ];
static unsigned int cnt_of[ 10 ];

static unsigned int plain_tree( unsigned int n ) {
  unsigned int l = 0U, m = n;
  while( m > 1U ) {
    cnt_of[ l ] = m;
    for( unsigned int j=0U; j<m; j+=2U ) {
      if( j + 1U < m ) { who[ l ][ j ] = j + 1U; who[ l ][ j + 1U ] = j; }
      else               who[ l ][ j ] = j;
    }
    m = ( m + 1U ) / 2U;
    l++;
  }
  cnt_of[ l ] = 1U;
  return l;
}

static void check_shape( void ) {
  CHECK( fd_fec_depth( 1U ) == 0U && fd_fec_depth( 2U ) == 1U && fd_fec_depth( 3U ) == 2U && fd_fec_depth( 4U ) == 2U );
  CHECK( fd_fec_depth( 5U ) == 3U && fd_fec_depth( 64U ) == 6U && fd_fec_depth( 65U ) == 7U && fd_fec_depth( 256U ) == 8U );
  for( unsigned int n=1U; n<=FD_FEC_LEAF_MAX; n++ ) {
    unsigned int D = plain_tree( n );
    CHECK( fd_fec_depth( n ) == D );
    /* floor( log2( n - 1 ) ) + 1 */
    if( n > 1U ) { unsigned int lg = 0U; while( ( ( n - 1U ) >> ( lg + 1U ) ) != 0U ) lg++; CHECK( D == lg + 1U ); }
    unsigned int total = 0U;
    for( unsigned int l=0U; l<=D; l++ ) {
      CHECK( fd_fec_layer_cnt( n, l ) == cnt_of[ l ] );
      if( l < D ) total += cnt_of[ l ];
    }
    CHECK( total <= 510U );                                   /* what the kernel keeps under the root */
    CHECK( total <= fd_fec_node_cap( 64U * ( ( n + 63U ) / 64U ) ) );   /* ... in a block of whole wavefronts */
    for( unsigned int j=0U; j<n; j++ )
      for( unsigned int l=0U; l<D; l++ ) {
        unsigned int s = fd_fec_sibling( j, l, n );
        CHECK( s == who[ l ][ j >> l ] );
        CHECK( s < cnt_of[ l ] );
      }
  }
}

/* ---- the descriptor ------------------------------------------------------------------------------------------ */

static void check_set( void ) {
  unsigned int const NO = FD_SHRED_NO_SIG;
  CHECK(  fd_fec_set_bad( 0U, 0U,   NO, 0U, 1000UL, 0UL, 0UL ) );
  CHECK( !fd_fec_set_bad( 0U, 1U,   NO, 0U, 1000UL, 0UL, 0UL ) );
  CHECK( !fd_fec_set_bad( 0U, 256U, NO, 0U, 1000UL, 0UL, 0UL ) );
  CHECK(  fd_fec_set_bad( 0U, 257U, NO, 0U, 1000UL, 0UL, 0UL ) );
  CHECK(  fd_fec_set_bad( 0U, 0xFFFFU, NO, 0U, 100000UL, 0UL, 0UL ) );
  /* the member range: ending at the array's end is good; no wrap near 2^32 */
  CHECK( !fd_fec_set_bad( 936U, 64U, NO, 0U, 1000UL, 0UL, 0UL ) );
  CHECK(  fd_fec_set_bad( 937U, 64U, NO, 0U, 1000UL, 0UL, 0UL ) );
  CHECK(  fd_fec_set_bad( 0xFFFFFFFFU, 1U, NO, 0U, 1000UL, 0UL, 0UL ) );
  CHECK(  fd_fec_set_bad( 0xFFFFFFFFU, 2U, NO, 0U, 0x100000000UL, 0UL, 0UL ) );
  CHECK( !fd_fec_set_bad( 0xFFFFFFFFU, 2U, NO, 0U, 0x100000001UL, 0UL, 0UL ) );
  CHECK(  fd_fec_set_bad( 0U, 1U, NO, 0U, 0UL, 0UL, 0UL ) );
  /* the key and the slot, by the shreds rule */
  CHECK( !fd_fec_set_bad( 0U, 1U, 3U, 0U, 1UL, 4UL, 1UL ) );
  CHECK(  fd_fec_set_bad( 0U, 1U, 4U, 0U, 1UL, 4UL, 1UL ) );
  CHECK(  fd_fec_set_bad( 0U, 1U, 0U, 0U, 1UL, 0UL, 1UL ) );
  CHECK( !fd_fec_set_bad( 0U, 1U, 0xFFFEU, 0U, 1UL, 0xFFFFUL, 1UL ) );
  CHECK( !fd_fec_set_bad( 0U, 1U, NO, 0U, 1UL, 0x10000UL, 1UL ) );
  CHECK( !fd_fec_set_bad( 0U, 1U, 0U, 6U, 1UL, 1UL, 7UL ) );
  CHECK(  fd_fec_set_bad( 0U, 1U, 0U, 7U, 1UL, 1UL, 7UL ) );
  CHECK(  fd_fec_set_bad( 0U, 1U, 0U, 0U, 1UL, 1UL, 0UL ) );
  CHECK( !fd_fec_set_bad( 0U, 1U, NO, 0xFFFFFFFFU, 1UL, 0UL, 0UL ) );
}

static void check_range( void ) {
  unsigned long const A = 1UL << 20;
  CHECK( !fd_fec_range_bad( (unsigned)A - 1203U, A, 0, 0U ) );
  CHECK(  fd_fec_range_bad( (unsigned)A - 1202U, A, 0, 0U ) );
  CHECK(  fd_fec_range_bad( 0xFFFFFFFFU, A, 0, 0U ) );
  CHECK(  fd_fec_range_bad( 0xFFFFFFFFU, 0x100000000UL + 1201UL, 0, 0U ) );
  CHECK( !fd_fec_range_bad( 0xFFFFFFFFU, 0x100000000UL + 1202UL, 0, 0U ) );
  /* a data shred needs 1203 bytes, a code shred 1228; any other variant is not a code shred */
  static unsigned int const data[] = { 0x80U, 0x96U, 0xb6U, 0xa5U, 0x00U, 0xffU }, code[] = { 0x46U, 0x66U, 0x76U, 0x5aU & 0x4fU };
  for( unsigned int k=0U; k<6U; k++ ) CHECK( !fd_fec_range_bad( (unsigned)A - 1203U, A, 1, data[k] ) );
  for( unsigned int k=0U; k<4U; k++ ) {
    CHECK(  fd_fec_range_bad( (unsigned)A - 1203U, A, 1, code[k] ) );
    CHECK(  fd_fec_range_bad( (unsigned)A - 1227U, A, 1, code[k] ) );
    CHECK( !fd_fec_range_bad( (unsigned)A - 1228U, A, 1, code[k] ) );
  }
  CHECK( fd_fec_range_bad( (unsigned)A - 1202U, A, 1, 0x80U ) );
}

/* ---- the members ---------------------------------------------------------------------------------------------- */

typedef struct { unsigned char b[ 28 ]; } hdr_t;

static void put( hdr_t * h, unsigned int at, unsigned long v, unsigned int n ) {
  for( unsigned int k=0U; k<n; k++ ) h->b[ at - 0x40U + k ] = (unsigned char)( v >> ( 8U * k ) );
}

/* member j of a set of data_cnt + code_cnt leaves of the class of data type t (0x80, 0x90, 0xb0) */
static hdr_t member_hdr( unsigned int t, unsigned int data_cnt, unsigned int code_cnt, unsigned int j ) {
  unsigned int D = fd_fec_depth( data_cnt + code_cnt );
  hdr_t h; memset( &h, 0xEE, sizeof(h) );
  put( &h, 0x41U, 1000UL, 8U ); put( &h, 0x4dU, 0x1234UL, 2U ); put( &h, 0x4fU, 320UL, 4U );
  if( j < data_cnt ) {
    put( &h, 0x40U, t | D, 1U ); put( &h, 0x49U, 320UL + j, 4U );
    put( &h, 0x53U, 3UL, 2U ); put( &h, 0x55U, 0UL, 1U ); put( &h, 0x56U, 500UL, 2U );
  } else {
    put( &h, 0x40U, fd_fec_type_mate( t ) | D, 1U ); put( &h, 0x49U, 700UL + j, 4U );
    put( &h, 0x53U, data_cnt, 2U ); put( &h, 0x55U, code_cnt, 2U ); put( &h, 0x57U, j - data_cnt, 2U );
  }
  return h;
}

static void words( hdr_t const * h, unsigned int * w ) {
  for( int k=0; k<FD_SHRED_FIELD_WORDS; k++ )
    w[k] = (unsigned int)h->b[4*k] | ( (unsigned int)h->b[4*k+1] << 8 ) | ( (unsigned int)h->b[4*k+2] << 16 ) | ( (unsigned int)h->b[4*k+3] << 24 );
}

/* member h held against member 0 h0 and the first code member hc, as position j of cnt */
static int member_bad( hdr_t const * h, hdr_t const * h0, hdr_t const * hc, unsigned int j, unsigned int cnt, fd_shred_info_t * info ) {
  unsigned int w[ FD_SHRED_FIELD_WORDS ], w0[ FD_SHRED_FIELD_WORDS ], wc[ FD_SHRED_FIELD_WORDS ];
  fd_shred_fields_t f, f0, fc;
  words( h, w ); words( h0, w0 ); words( hc, wc );
  fd_shred_fields( w, &f ); fd_shred_fields( w0, &f0 ); fd_shred_fields( wc, &fc );
  return fd_fec_member_bad( &f, fd_fec_version( w ), &f0, fd_fec_version( w0 ), &fc, j, cnt, info );
}

static void check_members( void ) {
  static unsigned int const types[] = { 0x80U, 0x90U, 0xb0U };
  static unsigned int const split[][2] = { { 1U, 1U }, { 2U, 1U }, { 32U, 32U }, { 17U, 16U }, { 67U, 67U }, { 128U, 128U }, { 1U, 255U }, { 255U, 1U } };
  fd_shred_info_t in;
  unsigned int w[ FD_SHRED_FIELD_WORDS ];
  hdr_t v = member_hdr( 0x80U, 2U, 2U, 0U );
  put( &v, 0x4dU, 0xBEEFUL, 2U ); words( &v, w );
  CHECK( fd_fec_version( w ) == 0xBEEFU );
  CHECK( fd_fec_type_mate( 0x80U ) == 0x40U && fd_fec_type_mate( 0x60U ) == 0x90U && fd_fec_type_mate( 0x70U ) == 0xb0U );
  CHECK( fd_fec_type_mate( 0xa0U ) > 0xf0U && fd_fec_type_mate( 0x50U ) > 0xf0U );
  for( unsigned int t=0U; t<3U; t++ ) for( unsigned int s=0U; s<8U; s++ ) {
    unsigned int dc = split[s][0], cc = split[s][1], n = dc + cc, D = fd_fec_depth( n );
    hdr_t h0 = member_hdr( types[t], dc, cc, 0U ), hc = member_hdr( types[t], dc, cc, dc );
    /* a consistent set: every member passes, and its info is its place */
    for( unsigned int j=0U; j<n; j++ ) {
      hdr_t h = member_hdr( types[t], dc, cc, j );
      CHECK( !member_bad( &h, &h0, &hc, j, n, &in ) );
      CHECK( in.leaf == j && in.depth == D );
      CHECK( in.moff == ( j < dc ? 1203U : 1228U ) - 20U * D - ( types[t] == 0xb0U ? 64U : 0U ) );
    }
    unsigned int at[3] = { 0U, n / 2U, n - 1U };
    for( unsigned int a=0U; a<3U; a++ ) {
      unsigned int j = at[a];
      hdr_t g = member_hdr( types[t], dc, cc, j ), h;
      int data = j < dc;
      /* the position */
      CHECK( member_bad( &g, &h0, &hc, j + 1U, n, &in ) );
      if( j ) CHECK( member_bad( &g, &h0, &hc, j - 1U, n, &in ) );
      /* the depth: one more, one less */
      h = g; put( &h, 0x40U, g.b[0] + 1U, 1U );              CHECK( member_bad( &h, &h0, &hc, j, n, &in ) );
      if( D ) { h = g; put( &h, 0x40U, g.b[0] - 1U, 1U );    CHECK( member_bad( &h, &h0, &hc, j, n, &in ) ); }
      /* slot, version, fec_set_idx: one up, one down (a data member's idx moves with fec_set_idx, so its leaf stays) */
      h = g; put( &h, 0x41U, 1001UL, 8U );                    CHECK( member_bad( &h, &h0, &hc, j, n, &in ) );
      h = g; put( &h, 0x41U, 999UL, 8U );                     CHECK( member_bad( &h, &h0, &hc, j, n, &in ) );
      h = g; put( &h, 0x41U, 1000UL | ( 1UL << 40 ), 8U );    CHECK( member_bad( &h, &h0, &hc, j, n, &in ) );
      h = g; put( &h, 0x4dU, 0x1235UL, 2U );                  CHECK( member_bad( &h, &h0, &hc, j, n, &in ) );
      h = g; put( &h, 0x4dU, 0x1334UL, 2U );                  CHECK( member_bad( &h, &h0, &hc, j, n, &in ) );
      h = g; put( &h, 0x4fU, 321UL, 4U ); if( data ) put( &h, 0x49U, 321UL + j, 4U );
                                                              CHECK( member_bad( &h, &h0, &hc, j, n, &in ) );
      h = g; put( &h, 0x4fU, 319UL, 4U ); if( data ) put( &h, 0x49U, 319UL + j, 4U );
                                                              CHECK( member_bad( &h, &h0, &hc, j, n, &in ) );
      /* the type: the two other classes, same kind; a type that is none */
      for( unsigned int u=0U; u<3U; u++ ) {
        unsigned int ty = data ? types[u] : fd_fec_type_mate( types[u] );
        h = g; put( &h, 0x40U, ty | D, 1U );
        CHECK( member_bad( &h, &h0, &hc, j, n, &in ) == ( u != t ) );
      }
      h = g; put( &h, 0x40U, 0xa0U | D, 1U );                 CHECK( member_bad( &h, &h0, &hc, j, n, &in ) );
      if( data ) {
        /* parent_off (both values parse: slot 1000) */
        h = g; put( &h, 0x53U, 4UL, 2U );                     CHECK( member_bad( &h, &h0, &hc, j, n, &in ) );
        h = g; put( &h, 0x53U, 2UL, 2U );                     CHECK( member_bad( &h, &h0, &hc, j, n, &in ) );
      } else {
        /* data_cnt + code_cnt = cnt: the sum off by one either way; the sum kept and the split moved (code.idx
           follows data_cnt so that the leaf stays j) */
        if( dc + cc < 256U ) { h = g; put( &h, 0x55U, cc + 1U, 2U );   CHECK( member_bad( &h, &h0, &hc, j, n, &in ) ); }
        if( cc > j - dc + 1U ) { h = g; put( &h, 0x55U, cc - 1U, 2U ); CHECK( member_bad( &h, &h0, &hc, j, n, &in ) ); }
        CHECK( member_bad( &g, &h0, &hc, j, n + 1U, &in ) );
        if( j - dc >= 1U ) {
          h = g; put( &h, 0x53U, dc + 1U, 2U ); put( &h, 0x55U, cc - 1U, 2U ); put( &h, 0x57U, j - dc - 1U, 2U );
          CHECK( member_bad( &h, &h0, &hc, j, n, &in ) );
          CHECK( !member_bad( &h, &h0, &h, j, n, &in ) );    /* (it is the disagreement that is refused) */
        }
        if( dc > 1U ) {
          h = g; put( &h, 0x53U, dc - 1U, 2U ); put( &h, 0x55U, cc + 1U, 2U ); put( &h, 0x57U, j - dc + 1U, 2U );
          CHECK( member_bad( &h, &h0, &hc, j, n, &in ) );
        }
      }
    }
    /* a code shred in front: as leaf 0 it fails whatever it says */
    hdr_t c0 = member_hdr( types[t], dc, cc, dc );
    CHECK( member_bad( &c0, &c0, &c0, 0U, n, &in ) );
  }
  /* one leaf: depth 0, a data shred alone */
  hdr_t one = member_hdr( 0x90U, 1U, 0U, 0U );
  CHECK( !member_bad( &one, &one, &one, 0U, 1U, &in ) && in.depth == 0U && in.moff == 1203U );
  /* the words */
  unsigned int a[ 16 ], b[ 16 ];
  for( unsigned int k=0U; k<16U; k++ ) a[k] = b[k] = 0x01010101U * k;
  CHECK( !fd_fec_words_differ( a, b, 16U ) );
  for( unsigned int k=0U; k<16U; k++ ) {
    b[k] ^= 1U << ( k + 3U );
    CHECK( fd_fec_words_differ( a, b, 16U ) && fd_fec_words_differ( a, b, k + 1U ) && !fd_fec_words_differ( a, b, k ) );
    b[k] = a[k];
  }
}

int main( void ) {
  check_shape();
  check_set();
  check_range();
  check_members();
  if( fails ) { fprintf( stderr, "%d checks failed\n", fails ); return 1; }
  puts( "ok" );
  return 0;
}
