#pragma once
/* fd_gpu_sha256.h -- SHA-256 with one message per lane (CDNA4 device code).

   The GPU side of the reference's fd_sha256 (src/ballet/sha256/fd_sha256.c) for the two hashes a Merkle
   shred's root needs (src/ballet/bmtree/fd_bmtree.c: fd_bmtree_hash_leaf and the 20-byte merge with the long
   prefixes), and for any batch of messages (fd_sha256_batch_kernel).  Every lane hashes its own message: the
   eight state words and the 16-word schedule are VGPRs, the 64 rounds are fully unrolled with the round constants
   as literals (nothing is indexed at run time, so nothing goes to scratch), rotations are v_alignbit_b32, the
   3-way xors, Ch and Maj are one v_bitop3_b32 each.  Messages are read where they lie, at any byte alignment,
   with aligned dword loads + v_alignbyte_b32 (fd_load_words, fd_gpu_sha512.h); padding and the length are made
   in registers. */

#include "fd_gpu_sha512.h"

FD_DEV u32 fd_rotr32( u32 x, int n ) { return __builtin_amdgcn_alignbit( x, x, (u32)n ); }
FD_DEV u32 fd_xor3_32( u32 x, u32 y, u32 z ) { return __builtin_amdgcn_bitop3_b32( x, y, z, 0x96 ); }
/* Ch as v_bitop3_b32 (truth table 0xca), not the compiler's v_bfi_b32, for the reason fd_ch64 gives */
FD_DEV u32 fd_ch32(  u32 x, u32 y, u32 z ) { return __builtin_amdgcn_bitop3_b32( x, y, z, 0xca ); }
FD_DEV u32 fd_maj32( u32 x, u32 y, u32 z ) { return __builtin_amdgcn_bitop3_b32( x, y, z, 0xe8 ); }

#define FD_SHA256_K_LIST \
  0x428a2f98U, 0x71374491U, 0xb5c0fbcfU, 0xe9b5dba5U, 0x3956c25bU, 0x59f111f1U, 0x923f82a4U, 0xab1c5ed5U, \
  0xd807aa98U, 0x12835b01U, 0x243185beU, 0x550c7dc3U, 0x72be5d74U, 0x80deb1feU, 0x9bdc06a7U, 0xc19bf174U, \
  0xe49b69c1U, 0xefbe4786U, 0x0fc19dc6U, 0x240ca1ccU, 0x2de92c6fU, 0x4a7484aaU, 0x5cb0a9dcU, 0x76f988daU, \
  0x983e5152U, 0xa831c66dU, 0xb00327c8U, 0xbf597fc7U, 0xc6e00bf3U, 0xd5a79147U, 0x06ca6351U, 0x14292967U, \
  0x27b70a85U, 0x2e1b2138U, 0x4d2c6dfcU, 0x53380d13U, 0x650a7354U, 0x766a0abbU, 0x81c2c92eU, 0x92722c85U, \
  0xa2bfe8a1U, 0xa81a664bU, 0xc24b8b70U, 0xc76c51a3U, 0xd192e819U, 0xd6990624U, 0xf40e3585U, 0x106aa070U, \
  0x19a4c116U, 0x1e376c08U, 0x2748774cU, 0x34b0bcb5U, 0x391c0cb3U, 0x4ed8aa4aU, 0x5b9cca4fU, 0x682e6ff3U, \
  0x748f82eeU, 0x78a5636fU, 0x84c87814U, 0x8cc70208U, 0x90befffaU, 0xa4506cebU, 0xbef9a3f7U, 0xc67178f2U

FD_DEV void fd_sha256_init( u32 h[ 8 ] ) {
  h[0] = 0x6a09e667U; h[1] = 0xbb67ae85U; h[2] = 0x3c6ef372U; h[3] = 0xa54ff53aU;
  h[4] = 0x510e527fU; h[5] = 0x9b05688cU; h[6] = 0x1f83d9abU; h[7] = 0x5be0cd19U;
}

/* One 64-byte block: w = its 16 big-endian words (destroyed: the schedule is expanded in place) */
FD_DEV void fd_sha256_block( u32 h[ 8 ], u32 w[ 16 ] ) {
  constexpr u32 K[ 64 ] = { FD_SHA256_K_LIST };
  u32 a=h[0], b=h[1], c=h[2], d=h[3], e=h[4], f=h[5], g=h[6], hh=h[7];
#pragma unroll
  for( int t=0; t<64; t++ ) {
    int r = t & 15;
    if( t >= 16 ) {
      u32 w15 = w[(r+1)&15], w2 = w[(r+14)&15];
      u32 s0 = fd_xor3_32( fd_rotr32( w15,  7 ), fd_rotr32( w15, 18 ), w15 >>  3 );
      u32 s1 = fd_xor3_32( fd_rotr32( w2,  17 ), fd_rotr32( w2,  19 ), w2  >> 10 );
      w[r] += s0 + w[(r+9)&15] + s1;
    }
    u32 S1 = fd_xor3_32( fd_rotr32( e, 6 ), fd_rotr32( e, 11 ), fd_rotr32( e, 25 ) );
    u32 t1 = hh + S1 + fd_ch32( e, f, g ) + K[t] + w[r];
    u32 S0 = fd_xor3_32( fd_rotr32( a, 2 ), fd_rotr32( a, 13 ), fd_rotr32( a, 22 ) );
    u32 mj = fd_maj32( a, b, c );
    hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + S0 + mj;
  }
  h[0]+=a; h[1]+=b; h[2]+=c; h[3]+=d; h[4]+=e; h[5]+=f; h[6]+=g; h[7]+=hh;
}

/* Block b (of nb) of a message of L < 2^29 bytes whose byte j is p[j], as 16 big-endian words with the padding
   and the length.  A block that holds no message byte loads nothing; one that holds any loads 17 aligned
   dwords from the dword of p + 64 b on: up to 67 bytes past the message's end. */
FD_DEV void fd_sha256_msg_block( u32 w[ 16 ], unsigned char const * p, u32 b, u32 nb, u32 L ) {
  if( 64u*b < L ) fd_load_words<16>( w, p + 64u*b );
  else {
#pragma unroll
    for( int i=0; i<16; i++ ) w[i] = 0u;
  }
#pragma unroll
  for( int i=0; i<16; i++ ) w[i] = fd_bswap32( w[i] );
  if( 64u*(b+1u) > L ) {                          /* the message ends in this block or before it: mask, pad, length */
#pragma unroll
    for( int i=0; i<16; i++ ) {
      int nv = (int)L - (int)( 64u*b ) - 4*i;     /* message bytes in this word */
      u32 x  = w[i];
      u32 m  = nv>=4 ? ~0u : ( nv<=0 ? 0u : ( ~0u << ( 8*( 4-nv ) ) ) );
      x &= m;
      if( nv>=0 && nv<4 ) x |= 0x80u << ( 8*( 3-nv ) );
      if( b==nb-1u && i==15 ) x = L << 3;
      if( b==nb-1u && i==14 ) x = 0u;
      w[i] = x;
    }
  }
}

FD_DEV u32 fd_sha256_blocks( u32 L ) { return ( L + 9u + 63u ) >> 6; }

/* SHA-256( M ) of msg_sz < 2^29 bytes at msg (any alignment) -> the state: 8 words whose big-endian bytes are
   the digest.  Reads up to 67 bytes past the message; the caller's buffer carries that slack. */
FD_DEV void fd_sha256_bytes( u32 h[ 8 ], unsigned char const * msg, u32 msg_sz ) {
  fd_sha256_init( h );
  u32 nb = fd_sha256_blocks( msg_sz );
#pragma unroll 1
  for( u32 b=0; b<nb; b++ ) {
    u32 w[16];
    fd_sha256_msg_block( w, msg, b, nb, msg_sz );
    fd_sha256_block( h, w );
  }
}

/* The 26-byte prefixes of the shred tree (fd_bmtree.c, FD_BMTREE_LONG_PREFIX_SZ): six big-endian words and the
   two bytes that open the seventh */
#define FD_BMTREE_PFX( c0, s ) { ((u32)(c0)<<24)|((u32)s[0]<<16)|((u32)s[1]<<8)|(u32)s[2],               \
    ((u32)s[3]<<24)|((u32)s[4]<<16)|((u32)s[5]<<8)|(u32)s[6],     ((u32)s[7]<<24)|((u32)s[8]<<16)|((u32)s[9]<<8)|(u32)s[10],   \
    ((u32)s[11]<<24)|((u32)s[12]<<16)|((u32)s[13]<<8)|(u32)s[14], ((u32)s[15]<<24)|((u32)s[16]<<16)|((u32)s[17]<<8)|(u32)s[18], \
    ((u32)s[19]<<24)|((u32)s[20]<<16)|((u32)s[21]<<8)|(u32)s[22], ((u32)s[23]<<24)|((u32)s[24]<<16) }

/* Leaf of the shred tree: SHA-256( 0x00 "SOLANA_MERKLE_SHREDS_LEAF" data[0, data_sz) ), data_sz >= 38.  The
   prefix is 26 bytes, so the message's byte j is (data - 26)[j]: the blocks are read from there, and block 0's
   first 26 bytes -- bytes in front of data, which the caller owns (a shred's signature) -- are replaced by the
   prefix.  Reads [data - 26 rounded down to a dword, data + data_sz + 67). */
FD_DEV void fd_sha256_shred_leaf( u32 h[ 8 ], unsigned char const * data, u32 data_sz ) {
  constexpr char s[] = "SOLANA_MERKLE_SHREDS_LEAF";
  constexpr u32 pfx[ 7 ] = FD_BMTREE_PFX( 0x00, s );
  fd_sha256_init( h );
  u32 L = 26u + data_sz, nb = fd_sha256_blocks( L );
#pragma unroll 1
  for( u32 b=0; b<nb; b++ ) {
    u32 w[16];
    fd_sha256_msg_block( w, data - 26, b, nb, L );
    if( b==0u ) {
#pragma unroll
      for( int i=0; i<6; i++ ) w[i] = pfx[i];
      w[6] = pfx[6] | ( w[6] & 0xffffu );
    }
    fd_sha256_block( h, w );
  }
}

/* One merge of the shred tree, in place: n = SHA-256( 0x01 "SOLANA_MERKLE_SHREDS_NODE" l r ), where l and r are
   the first 20 bytes of n and the 20 bytes s (5 big-endian words), n on the left if !right.  66 bytes: the
   second block is two data bytes, the padding and the length, nothing loaded. */
FD_DEV void fd_sha256_shred_merge( u32 n[ 8 ], u32 const s[ 5 ], int right ) {
  constexpr char str[] = "SOLANA_MERKLE_SHREDS_NODE";
  constexpr u32 pfx[ 7 ] = FD_BMTREE_PFX( 0x01, str );
  u32 x[ 10 ];
#pragma unroll
  for( int i=0; i<5; i++ ) { x[i] = right ? s[i] : n[i]; x[5+i] = right ? n[i] : s[i]; }
  u32 w[ 16 ];
#pragma unroll
  for( int i=0; i<6; i++ ) w[i] = pfx[i];
  w[6] = pfx[6] | ( x[0] >> 16 );
#pragma unroll
  for( int i=0; i<9; i++ ) w[7+i] = ( x[i] << 16 ) | ( x[i+1] >> 16 );
  fd_sha256_init( n );
  fd_sha256_block( n, w );
  w[0] = ( x[9] << 16 ) | 0x8000u;
#pragma unroll
  for( int i=1; i<15; i++ ) w[i] = 0u;
  w[15] = 66u * 8u;
  fd_sha256_block( n, w );
}
