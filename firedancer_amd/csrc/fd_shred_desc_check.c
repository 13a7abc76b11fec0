/* Stand-alone check of fd_shred_desc.h, the rules that give a Merkle shred descriptor (fdgpu_shred_desc_t) its code
   before any hashing: every descriptor, parse and Merkle rule one value on each side of its edge, the order of the
   rules, the field offsets against a header written byte by byte, and moff / leaf / depth of all six variants.
   firedancer_amd/build.py builds it and tests/test_shred_desc.py runs it; built with -fsanitize=address,undefined
   it also checks the reads of the word array.  Exit status 0 and "ok" on success. */

#include <stdio.h>
#include <string.h>
#include "fd_shred_desc.h"

static int fails;
#define CHECK( c ) do { if( !(c) ) { fprintf( stderr, "line %d: %s\n", __LINE__, #c ); fails++; } } while(0)

/* a shred header's bytes [0x40, 0x5c), written field by field at the offsets of src/ballet/shred/fd_shred.h */
typedef struct { unsigned char b[ 28 ]; } hdr_t;

static void put( hdr_t * h, unsigned int at, unsigned long v, unsigned int n ) {
  for( unsigned int k=0U; k<n; k++ ) h->b[ at - 0x40U + k ] = (unsigned char)( v >> ( 8U * k ) );
}

static hdr_t data_hdr( unsigned int variant, unsigned long slot, unsigned int idx, unsigned int fec, unsigned int parent_off,
                       unsigned int flags, unsigned int size ) {
  hdr_t h; memset( &h, 0xEE, sizeof(h) );
  put( &h, 0x40U, variant, 1U ); put( &h, 0x41U, slot, 8U ); put( &h, 0x49U, idx, 4U ); put( &h, 0x4dU, 0x1234UL, 2U );
  put( &h, 0x4fU, fec, 4U ); put( &h, 0x53U, parent_off, 2U ); put( &h, 0x55U, flags, 1U ); put( &h, 0x56U, size, 2U );
  return h;
}

static hdr_t code_hdr( unsigned int variant, unsigned int idx, unsigned int data_cnt, unsigned int code_cnt, unsigned int cidx ) {
  hdr_t h; memset( &h, 0xEE, sizeof(h) );
  put( &h, 0x40U, variant, 1U ); put( &h, 0x41U, 77UL, 8U ); put( &h, 0x49U, idx, 4U ); put( &h, 0x4dU, 0x1234UL, 2U );
  put( &h, 0x4fU, 3UL, 4U ); put( &h, 0x53U, data_cnt, 2U ); put( &h, 0x55U, code_cnt, 2U ); put( &h, 0x57U, cidx, 2U );
  return h;
}

static int classify( hdr_t const * h, unsigned int sz, unsigned int flags, fd_shred_info_t * info ) {
  unsigned int w[ FD_SHRED_FIELD_WORDS ];
  for( int k=0; k<FD_SHRED_FIELD_WORDS; k++ )
    w[k] = (unsigned int)h->b[4*k] | ( (unsigned int)h->b[4*k+1] << 8 ) | ( (unsigned int)h->b[4*k+2] << 16 ) | ( (unsigned int)h->b[4*k+3] << 24 );
  fd_shred_fields_t f;
  fd_shred_fields( w, &f );
  return fd_shred_classify( &f, sz, flags, info );
}

#define OK     0
#define PARSE  FD_SHRED_ERR_PARSE
#define MERKLE FD_SHRED_ERR_MERKLE

static void check_fields( void ) {
  hdr_t h = data_hdr( 0x96U, 0x0807060504030201UL, 0xA4A3A2A1U, 0xB4B3B2B1U, 0xC2C1U, 0xD1U, 0xE2E1U );
  unsigned int w[ FD_SHRED_FIELD_WORDS ];
  memcpy( w, h.b, sizeof(w) );                       /* (a little-endian host, as every target of the engine) */
  fd_shred_fields_t f;
  fd_shred_fields( w, &f );
  CHECK( f.variant == 0x96U && f.slot == 0x0807060504030201UL && f.idx == 0xA4A3A2A1U && f.fec_set_idx == 0xB4B3B2B1U );
  CHECK( f.h53 == 0xC2C1U && f.flags == 0xD1U && f.size == 0xE2E1U );
  h = code_hdr( 0x66U, 9U, 0xC2C1U, 0xD2D1U, 0xF2F1U );
  memcpy( w, h.b, sizeof(w) );
  fd_shred_fields( w, &f );
  CHECK( f.h53 == 0xC2C1U && f.h55 == 0xD2D1U && f.h57 == 0xF2F1U );
}

static void check_desc( void ) {
  unsigned long const A = 1UL << 20;
  /* the range: ending exactly at the arena's end is good, one byte further is bad; no wrap near 2^32 */
  CHECK( !fd_shred_desc_bad( (unsigned)A - 1203U, 1203U, FD_SHRED_NO_SIG, 0U, A, 0UL, 0UL ) );
  CHECK(  fd_shred_desc_bad( (unsigned)A - 1202U, 1203U, FD_SHRED_NO_SIG, 0U, A, 0UL, 0UL ) );
  CHECK( !fd_shred_desc_bad( (unsigned)A, 0U, FD_SHRED_NO_SIG, 0U, A, 0UL, 0UL ) );
  CHECK(  fd_shred_desc_bad( (unsigned)A + 1U, 0U, FD_SHRED_NO_SIG, 0U, A, 0UL, 0UL ) );
  CHECK(  fd_shred_desc_bad( 0xFFFFFFFFU, 0xFFFFU, FD_SHRED_NO_SIG, 0U, A, 0UL, 0UL ) );
  CHECK(  fd_shred_desc_bad( 0xFFFFFFFFU, 2U, FD_SHRED_NO_SIG, 0U, 0xFFFFFFFFUL, 0UL, 0UL ) );
  CHECK( !fd_shred_desc_bad( 0xFFFFFFFFU, 2U, FD_SHRED_NO_SIG, 0U, 0x100000001UL, 0UL, 0UL ) );
  CHECK(  fd_shred_desc_bad( 0U, 1U, FD_SHRED_NO_SIG, 0U, 0UL, 0UL, 0UL ) );
  /* the key: NO_SIG or below key_cnt */
  CHECK( !fd_shred_desc_bad( 0U, 1203U, 3U, 0U, A, 4UL, 1UL ) );
  CHECK(  fd_shred_desc_bad( 0U, 1203U, 4U, 0U, A, 4UL, 1UL ) );
  CHECK(  fd_shred_desc_bad( 0U, 1203U, 0U, 0U, A, 0UL, 1UL ) );
  CHECK(  fd_shred_desc_bad( 0U, 1203U, 0xFFFEU, 0U, A, 0xFFFEUL, 1UL ) );
  CHECK( !fd_shred_desc_bad( 0U, 1203U, 0xFFFEU, 0U, A, 0xFFFFUL, 1UL ) );
  CHECK( !fd_shred_desc_bad( 0U, 1203U, FD_SHRED_NO_SIG, 0U, A, 0x10000UL, 1UL ) );     /* 0xFFFF is never a key */
  /* the signature slot, only where one is wanted */
  CHECK( !fd_shred_desc_bad( 0U, 1203U, 0U, 6U, A, 1UL, 7UL ) );
  CHECK(  fd_shred_desc_bad( 0U, 1203U, 0U, 7U, A, 1UL, 7UL ) );
  CHECK(  fd_shred_desc_bad( 0U, 1203U, 0U, 0xFFFFFFFFU, A, 1UL, 7UL ) );
  CHECK(  fd_shred_desc_bad( 0U, 1203U, 0U, 0U, A, 1UL, 0UL ) );
  CHECK( !fd_shred_desc_bad( 0U, 1203U, FD_SHRED_NO_SIG, 0xFFFFFFFFU, A, 0UL, 0UL ) );
}

static void check_variants( void ) {
  /* moff = full - 20 d - 64 resigned; the six Merkle types at the depths of the reference's fixtures and at 0 and 9 */
  static unsigned int const types[ 6 ] = { 0x80U, 0x90U, 0xb0U, 0x40U, 0x60U, 0x70U };
  fd_shred_info_t in;
  for( unsigned int t=0U; t<6U; t++ ) for( unsigned int d=0U; d<16U; d++ ) {
    unsigned int ty = types[t], data = t < 3U, resigned = ( ty == 0xb0U ) | ( ty == 0x70U );
    unsigned int full = data ? 1203U : 1228U;
    hdr_t h = data ? data_hdr( ty | d, 10UL, 8U, 5U, 1U, 0U, 88U ) : code_hdr( ty | d, 8U, 32U, 32U, 1U );
    int rc = classify( &h, full, 0U, &in );
    CHECK( rc == ( d < 10U ? OK : MERKLE ) );
    if( !rc ) CHECK( in.depth == d && in.leaf == ( data ? 3U : 33U ) && in.moff == full - 20U * d - 64U * resigned );
    /* the resolver's rule */
    rc = classify( &h, full, FD_SHRED_STRICT_LEAF, &in );
    CHECK( rc == ( d < 10U && ( data ? 3U : 33U ) < ( 1U << d ) ? OK : MERKLE ) );
  }
  /* not a Merkle type: the legacy variants, which the reference parses, and the rest */
  static unsigned int const other[] = { 0xa5U, 0x5aU, 0x00U, 0x05U, 0x15U, 0x25U, 0x35U, 0x55U, 0xa6U, 0xc5U, 0xd5U, 0xe5U, 0xf5U, 0xffU };
  for( unsigned long k=0UL; k<sizeof(other)/sizeof(other[0]); k++ ) {
    hdr_t h = data_hdr( other[k], 10UL, 8U, 5U, 1U, 0U, 88U );
    CHECK( classify( &h, 1228U, 0U, &in ) == PARSE );
    h = code_hdr( other[k], 8U, 32U, 32U, 1U );
    CHECK( classify( &h, 1228U, 0U, &in ) == PARSE );
  }
}

static void check_data( void ) {
  fd_shred_info_t in;
  hdr_t h;
#define DATA( variant, slot, idx, fec, poff, flags, size, sz ) ( h = data_hdr( variant, slot, idx, fec, poff, flags, size ), classify( &h, sz, 0U, &in ) )
  /* sz */
  CHECK( DATA( 0x86U, 10UL, 8U, 5U, 1U, 0U, 88U,    0U ) == PARSE );
  CHECK( DATA( 0x86U, 10UL, 8U, 5U, 1U, 0U, 88U,   87U ) == PARSE );
  CHECK( DATA( 0x86U, 10UL, 8U, 5U, 1U, 0U, 88U,   88U ) == PARSE );      /* (a header alone: sz < 1203) */
  CHECK( DATA( 0x86U, 10UL, 8U, 5U, 1U, 0U, 88U, 1202U ) == PARSE );
  CHECK( DATA( 0x86U, 10UL, 8U, 5U, 1U, 0U, 88U, 1203U ) == OK );
  CHECK( DATA( 0x86U, 10UL, 8U, 5U, 1U, 0U, 88U, 1210U ) == OK );
  CHECK( DATA( 0x86U, 10UL, 8U, 5U, 1U, 0U, 88U, 0xFFFFU ) == OK );
  /* size: the header at least, and payload + trailer inside 1,203 */
  CHECK( DATA( 0x86U, 10UL, 8U, 5U, 1U, 0U, 87U, 1203U ) == PARSE );
  CHECK( DATA( 0x86U, 10UL, 8U, 5U, 1U, 0U, 1203U - 120U, 1203U ) == OK );
  CHECK( DATA( 0x86U, 10UL, 8U, 5U, 1U, 0U, 1204U - 120U, 1203U ) == PARSE );
  CHECK( DATA( 0x96U, 10UL, 8U, 5U, 1U, 0U, 1203U - 152U, 1203U ) == OK );
  CHECK( DATA( 0x96U, 10UL, 8U, 5U, 1U, 0U, 1204U - 152U, 1203U ) == PARSE );
  CHECK( DATA( 0xb6U, 10UL, 8U, 5U, 1U, 0U, 1203U - 216U, 1203U ) == OK );
  CHECK( DATA( 0xb6U, 10UL, 8U, 5U, 1U, 0U, 1204U - 216U, 1203U ) == PARSE );
  CHECK( DATA( 0x80U, 10UL, 8U, 5U, 1U, 0U, 1203U, 1203U ) == OK );
  CHECK( DATA( 0x80U, 10UL, 8U, 5U, 1U, 0U, 1204U, 1203U ) == PARSE );
  CHECK( DATA( 0x8fU, 10UL, 8U, 5U, 1U, 0U, 1203U - 300U, 1203U ) == MERKLE );   /* parses at depth 15; the tree refuses */
  CHECK( DATA( 0x8fU, 10UL, 8U, 5U, 1U, 0U, 1204U - 300U, 1203U ) == PARSE );    /* parse decides first */
  CHECK( DATA( 0x86U, 10UL, 8U, 5U, 1U, 0U, 0xFFFFU, 1203U ) == PARSE );
  /* flags: 0x80 without 0x40 */
  CHECK( DATA( 0x86U, 10UL, 8U, 5U, 1U, 0x80U, 88U, 1203U ) == PARSE );
  CHECK( DATA( 0x86U, 10UL, 8U, 5U, 1U, 0xBFU, 88U, 1203U ) == PARSE );
  CHECK( DATA( 0x86U, 10UL, 8U, 5U, 1U, 0x40U, 88U, 1203U ) == OK );
  CHECK( DATA( 0x86U, 10UL, 8U, 5U, 1U, 0xC0U, 88U, 1203U ) == OK );
  CHECK( DATA( 0x86U, 10UL, 8U, 5U, 1U, 0x7FU, 88U, 1203U ) == OK );
  /* parent_off against slot */
  CHECK( DATA( 0x86U, 10UL, 8U, 5U, 10U - 1U, 0U, 88U, 1203U ) == OK );
  CHECK( DATA( 0x86U, 10UL, 8U, 5U, 10U,      0U, 88U, 1203U ) == PARSE );  /* slot > 1, parent_off == slot */
  CHECK( DATA( 0x86U, 10UL, 8U, 5U, 11U,      0U, 88U, 1203U ) == PARSE );  /* parent_off > slot */
  CHECK( DATA( 0x86U, 10UL, 8U, 5U, 0U,       0U, 88U, 1203U ) == PARSE );  /* slot != 0, parent_off == 0 */
  CHECK( DATA( 0x86U,  0UL, 8U, 5U, 0U,       0U, 88U, 1203U ) == OK );
  CHECK( DATA( 0x86U,  0UL, 8U, 5U, 1U,       0U, 88U, 1203U ) == PARSE );
  CHECK( DATA( 0x86U,  1UL, 8U, 5U, 1U,       0U, 88U, 1203U ) == OK );
  CHECK( DATA( 0x86U,  1UL, 8U, 5U, 0U,       0U, 88U, 1203U ) == PARSE );
  CHECK( DATA( 0x86U,  2UL, 8U, 5U, 1U,       0U, 88U, 1203U ) == OK );
  CHECK( DATA( 0x86U,  2UL, 8U, 5U, 2U,       0U, 88U, 1203U ) == PARSE );
  CHECK( DATA( 0x86U, 0x100000000UL, 8U, 5U, 0xFFFFU, 0U, 88U, 1203U ) == OK );   /* the slot's high half counts */
  CHECK( DATA( 0x86U, 0x10000UL, 8U, 5U, 0xFFFFU, 0U, 88U, 1203U ) == OK );
  CHECK( DATA( 0x86U, 0xFFFFUL,  8U, 5U, 0xFFFFU, 0U, 88U, 1203U ) == PARSE );
  /* idx against fec_set_idx, and the leaf it gives */
  CHECK( DATA( 0x86U, 10UL, 5U, 5U, 1U, 0U, 88U, 1203U ) == OK && in.leaf == 0U );
  CHECK( DATA( 0x86U, 10UL, 4U, 5U, 1U, 0U, 88U, 1203U ) == PARSE );
  CHECK( DATA( 0x86U, 10UL, 0U, 0xFFFFFFFFU, 1U, 0U, 88U, 1203U ) == PARSE );
  CHECK( DATA( 0x86U, 10UL, 5U + 511U, 5U, 1U, 0U, 88U, 1203U ) == OK && in.leaf == 511U );
  CHECK( DATA( 0x86U, 10UL, 5U + 512U, 5U, 1U, 0U, 88U, 1203U ) == MERKLE );
  CHECK( DATA( 0x86U, 10UL, 0xFFFFFFFFU, 0U, 1U, 0U, 88U, 1203U ) == MERKLE );
  /* depth */
  CHECK( DATA( 0x89U, 10UL, 8U, 5U, 1U, 0U, 88U, 1203U ) == OK && in.depth == 9U );
  CHECK( DATA( 0x8aU, 10UL, 8U, 5U, 1U, 0U, 88U, 1203U ) == MERKLE );
  /* the strict leaf rule at 2^d */
  h = data_hdr( 0x86U, 10UL, 5U + 63U, 5U, 1U, 0U, 88U );
  CHECK( classify( &h, 1203U, FD_SHRED_STRICT_LEAF, &in ) == OK && in.leaf == 63U );
  h = data_hdr( 0x86U, 10UL, 5U + 64U, 5U, 1U, 0U, 88U );
  CHECK( classify( &h, 1203U, FD_SHRED_STRICT_LEAF, &in ) == MERKLE );
  CHECK( classify( &h, 1203U, 0U, &in ) == OK && in.leaf == 64U );
  h = data_hdr( 0x80U, 10UL, 5U, 5U, 1U, 0U, 88U );
  CHECK( classify( &h, 1203U, FD_SHRED_STRICT_LEAF, &in ) == OK );
  h = data_hdr( 0x80U, 10UL, 6U, 5U, 1U, 0U, 88U );
  CHECK( classify( &h, 1203U, FD_SHRED_STRICT_LEAF, &in ) == MERKLE );
  CHECK( classify( &h, 1203U, 2U, &in ) == OK );                            /* other flag bits mean nothing */
#undef DATA
}

static void check_code( void ) {
  fd_shred_info_t in;
  hdr_t h;
#define CODE( variant, idx, dc, cc, ci, sz ) ( h = code_hdr( variant, idx, dc, cc, ci ), classify( &h, sz, 0U, &in ) )
  /* sz */
  CHECK( CODE( 0x46U, 8U, 32U, 32U, 1U,   87U ) == PARSE );
  CHECK( CODE( 0x46U, 8U, 32U, 32U, 1U, 1203U ) == PARSE );
  CHECK( CODE( 0x46U, 8U, 32U, 32U, 1U, 1227U ) == PARSE );
  CHECK( CODE( 0x46U, 8U, 32U, 32U, 1U, 1228U ) == OK );
  CHECK( CODE( 0x46U, 8U, 32U, 32U, 1U, 1235U ) == OK );
  /* code.idx below code_cnt and not above idx */
  CHECK( CODE( 0x46U, 40U, 32U, 32U, 31U, 1228U ) == OK && in.leaf == 63U );
  CHECK( CODE( 0x46U, 40U, 32U, 32U, 32U, 1228U ) == PARSE );
  CHECK( CODE( 0x46U, 8U, 32U, 32U, 8U, 1228U ) == OK );
  CHECK( CODE( 0x46U, 8U, 32U, 32U, 9U, 1228U ) == PARSE );
  /* the counts */
  CHECK( CODE( 0x46U, 8U, 0U, 32U, 1U, 1228U ) == PARSE );
  CHECK( CODE( 0x46U, 8U, 1U, 1U, 0U, 1228U ) == OK && in.leaf == 1U );
  CHECK( CODE( 0x46U, 8U, 32U, 0U, 0U, 1228U ) == PARSE );
  CHECK( CODE( 0x49U, 8U, 1U, 255U, 1U, 1228U ) == OK );
  CHECK( CODE( 0x49U, 8U, 1U, 256U, 1U, 1228U ) == PARSE );                 /* the sum */
  CHECK( CODE( 0x49U, 8U, 0U, 256U, 1U, 1228U ) == PARSE );
  CHECK( CODE( 0x49U, 8U, 0U, 257U, 1U, 1228U ) == PARSE );
  CHECK( CODE( 0x49U, 8U, 128U, 128U, 1U, 1228U ) == OK );
  CHECK( CODE( 0x49U, 8U, 129U, 128U, 1U, 1228U ) == PARSE );
  CHECK( CODE( 0x49U, 8U, 0xFFFFU, 0xFFFFU, 1U, 1228U ) == PARSE );
  CHECK( CODE( 0x49U, 300U, 1U, 255U, 254U, 1228U ) == OK && in.leaf == 255U );   /* the largest leaf a code shred has */
  /* depth, and the strict rule */
  CHECK( CODE( 0x4aU, 8U, 32U, 32U, 1U, 1228U ) == MERKLE );
  h = code_hdr( 0x66U, 40U, 32U, 32U, 31U );
  CHECK( classify( &h, 1228U, FD_SHRED_STRICT_LEAF, &in ) == OK );
  h = code_hdr( 0x65U, 40U, 32U, 32U, 0U );
  CHECK( classify( &h, 1228U, FD_SHRED_STRICT_LEAF, &in ) == MERKLE );
  CHECK( classify( &h, 1228U, 0U, &in ) == OK && in.leaf == 32U );
#undef CODE
}

int main( void ) {
  check_fields();
  check_desc();
  check_variants();
  check_data();
  check_code();
  if( !fails ) puts( "ok" );
  return fails ? 1 : 0;
}
