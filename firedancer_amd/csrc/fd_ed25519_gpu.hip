/* fd_ed25519_gpu.hip -- MI355X (gfx950) batch ed25519 verify engine.

   256-thread workgroups, wave64.  Every batch (launch_batch) starts with
   fd_expand_kernel (txn -> signature map; raw-payload batches get it from
   fd_parse_kernel with the fd_txn_t image and the descriptor) and ends
   with fd_reduce_kernel (per transaction, the code of
   fd_ed25519_verify_batch_single_msg from its signatures' codes).  Between
   them one of three paths, by the batch's signature count, kernels in
   launch order:

   Latency path (launch_latency; at most FD_SMALL_BATCH_MAX signatures,
   which cannot fill the GPU).  fd_prep_kernel: roles by block, side by
   side -- decode A and its table [1..8](-A), decode R and [1..8](-R), and
   S < l, SHA-512(R||A||M), k mod l and the half-size pair (c0, c1) with
   s' = c1 S (fd_gpu_lattice.h), the hash on a quad of lanes for the
   smallest batches.  Then the walk [s']B + [c0](-A) + [c1](-R) == O over
   128 doublings on 8, 4, 2 or 1 lanes per signature as the batch grows:
   fd_dsm8_kernel, fd_dsm4_kernel, fd_dsm2_kernel, or fd_dsmh_kernel with
   fd_dsm_slowl_kernel; each runs the result-code procedure and, for the
   few signatures without a short pair, the full-length walk.  Without
   half-size scalars (half = 0): fd_prep_kernel, fd_table_kernel ahead of
   the one-lane walk, and [k](-A) + [S]B over 252 doublings compared with
   the decoded R in fd_dsm4_kernel, fd_dsm2_kernel or fd_dsm_kernel.

   Half-size throughput path (launch_half).
   fd_keydedup_kernel: a representative signature per distinct public key.
   fd_keysplit_kernel: the signatures of keys the batch repeats ordered
   ahead of the others.  fd_decode_kernel: roles by block, A and its table
   for the representatives, R and its table for every signature.
   fd_hashh_kernel: result codes, SHA-512, (c0, c1, s') as signed digits,
   and the repeated keys' high tables [2^68](-A), [2^136](-A).
   fd_dsmh_kernel: the walk, -A entries gathered at the representative's
   index, 128 doublings, or 64 over the high tables for a repeated key's
   signatures; base-point adds from the [0..32768]([2^e]B) affine tables
   (L2 / Infinity Cache resident).  fd_dsm_slow_kernel: what the walk's
   first blocks left of the signatures without a short pair.  A key with
   FD_FB_MIN signatures in the batch is treated like the base point
   (DESIGN 16): fd_keyclass_kernel picks those keys, fd_ftab_kernel builds
   their comb tables, their signatures get no lattice reduction, no decode
   of R and no -R table, walk 24 doublings in fd_dsmh_kernel's third body,
   and the full-length path's R-check kernels compare P with R's bytes.

   Full-length throughput path (launch_full; half = 0).  fd_decode_kernel
   (A only), fd_hash_kernel (signed radix-16 digits of k, radix-2^16 of
   S), fd_table_kernel, fd_dsm_kernel (252 doublings, 64 table adds
   prefetched one window ahead, 16 base-point adds), then R is compared
   without decoding it: fd_rprod_kernel, fd_rinv_kernel, fd_rcheck_kernel,
   fd_rslow_kernel.

   Replaces (behaviour, not code) fd_ed25519_verify /
   fd_ed25519_verify_batch_single_msg (src/ballet/ed25519/
   fd_ed25519_user.c:135-310) as called from fd_txn_verify
   (src/disco/verify/fd_verify_tile.h:59-108).

   Fixed windows instead of the reference's sliding wNAF
   (fd_curve25519.c:109-153): every lane of a wave performs the same
   doubling/add sequence, so SIMT lanes never diverge in the hot loop;
   only the table index is data dependent. */

#include "fd_gpu_sha512.h"
#include "fd_gpu_sha256.h"
#include "fd_gpu_curve.h"
#include "fd_gpu_txn.h"
#include "fd_gpu_lattice.h"
#include "fd_pin_list.h"
#include "../../include/fd_ed25519_gpu.h"

#include <hip/hip_runtime.h>
#include <atomic>
#include <mutex>
#include <string.h>
#include <stdio.h>
#include <time.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include <deque>
#include <thread>
#include <pthread.h>
#include <sched.h>

#define FD_WG 256
#define FD_ATAB_ENTRIES 9          /* [0..8](-A), cached form, 128 B each */
#define FD_ATAB_STORED  8          /* [1..8] stored per signature; [0] (the identity) is one shared constant line */
/* Base-point window, fixed at 16 bits: [0..32768]B, affine precomp, 96 B
   each (3.1 MB, L2 / Infinity-Cache resident) in HBM, gathered per lane
   one window ahead and added every 4th A window (16 adds).  Every walk and
   the [2^72]B, [2^120]B, [2^140]B, [2^196]B tables assume this width. */
#define FD_BWIN 16
#define FD_BTAB_ENTRIES 32769
#define FD_BDIG ( 256 / FD_BWIN )  /* signed radix-2^FD_BWIN digits of S */
#define FD_ARENA_SLACK  512UL      /* readable bytes past the last payload */

/* Path thresholds, in signatures per batch (defaults of the runtime overrides in fdgpu_debug_opts_t). */
/* Throughput path with half-size scalars (fd_gpu_lattice.h): 128 doublings
   instead of 252; 0 = the full-length walk with the deferred R check */
#define FD_HALF 1
/* Batches of at most this many signatures take the latency path
   (fd_prep_kernel, R decoded up front): they cannot fill the GPU, so
   per-wave instruction streams, not total work, set their time. */
#define FD_SMALL_BATCH_MAX 65536UL
/* fd_dsm_kernel without the carry fold (fd_gpu_f25519.h) for batches of at
   most this many signatures: <= 2 waves per SIMD, where the per-wave chain
   latency, not the instruction count, sets the time */
#define FD_NOFOLD_MAX 131072UL
#define FD_DSM8_MAX 8192UL           /* latency path: eight lanes per signature up to here, */
#define FD_DSM4_MAX 16384UL          /* four up to here, */
#define FD_DSM2_MAX 32768UL          /* then two up to here, then one (fd_dsm_kernel, R compared at its end) */
#define FD_QSHA_MAX 8192UL           /* latency path: the prep's hash role on a quad of lanes per signature up to here
                                        (fd_sha512_RAM_quad; 6 sg workgroups stay under one wave per SIMD) */

#define FD_STAGE_CHUNK ( 1UL << 20 )   /* host-staged batches: bytes per memcpy / H2D step */
/* gathered batches: the fd_txn_t image of the last record may end this far past its record */
#define FD_IMG_TAIL    1024UL
#define FD_PIPE_SUB    ( 1UL << 17 )   /* host batches of >= 2 FD_PIPE_SUB txns: sub-batches overlap H2D and kernels */
#define FD_PIPE_MAX    16UL
#define FD_PEND_ASMALL 2           /* per-signature code in flight: A small order, R's decode picks ERR_SIG / ERR_PUBKEY */
#define FD_PEND_REQ    3           /* per-signature code in flight: P's encoding != R's bytes -> decode R, compare */
#define FD_PEND_SLOW   4           /* per-signature code in flight: no half-size scalars, full 253-bit walk (fd_dsm_slow_kernel) */
#define FD_HDIG 40                 /* signed radix-16 digits of c0, c1 (< 2^159); the walk stops at the wave's top one */
#define FD_PSTAT_SLOW 0x80u        /* A-status bit: the signature is on the half-size path's slow list */
/* fd_keydedup_kernel: workgroups (of sg) whose lanes still look their keys up when the batch before had
   mostly distinct keys -- the sample that decides for the batch after */
#define FD_KD_SBLK( sg ) ( (sg) >> 4 ? (sg) >> 4 : 1u )

/* Repeated keys (fd_keysplit_kernel): a key with at least this many signatures in a batch is hot.  Its
   two high tables cost about 0.7 of a cold walk (chains of 68 and 136 doublings, two 8-entry tables) and buy a
   quarter of a walk per signature: break-even near 3 */
#define FD_HOT_MIN 8u
#define FD_KS_W    FD_LAT_SKEW_W     /* windows per part of a hot signature's c0 (fd_gpu_lattice.h) */
#define FD_KS_NW   FD_LAT_SKEW_NW    /* windows stored for it: digA rows [0, 2 W + NW), digR rows [0, NW) */

/* Fixed-base keys: a key with at least this many signatures in a batch gets comb tables of its own,
   FD_FB_T tables of [1..FD_FB_E]( [2^(32 t)](-A) ) in affine precomputed form (96 B an entry, 96 KB for the eight), and its
   signatures walk 24 doublings.  Reasoned, not measured: the tables cost about 1,100 field multiplies of wave
   time per key (the chain of up to 224 doublings shared by 8 keys of a wave, two waves of entries with an
   inversion each) and a signature saves about 880 / 64 of that, which puts the break-even near 80 signatures.
   Measured (tools/keyfixed_mix.py): a batch of keys with exactly 64 signatures each loses 0.42 ms per
   1M with the bound at 64, one of exactly 128 wins at 128 -- by 0.5 ms, with only half of its 8,192 keys under
   FD_FB_CAP.  A build with -DFD_FB_MIN=... measures another bound. */
#ifndef FD_FB_MIN
#define FD_FB_MIN  128u
#endif
#define FD_FB_T    8
#define FD_FB_E    128
/* A slot of the key cache has room for FD_FB_NT = 32 tables (fd_gpu_lattice.h), one per byte of k: table j =
   [1..128]( [2^(8j)](-A) ), 384 KB a slot.  A claim builds group 0, the FD_FB_T tables j = 0 (mod 4) above; a key found
   resident in a later batch is promoted (fd_keyclass_kernel), groups 1..3 are built, and its signatures then walk
   no doubling at all (dsmf_full). */
#define FD_FB_CAP  4096u              /* the most fixed-base keys of a batch (1.5 GiB of slots); a key beyond stays hot */
#define FD_FB_NONE 0xffffffffu        /* fidx[] of a representative whose key is not fixed-base */
#define FD_PEND_FBREQ 5               /* per-signature code in flight: a fixed-base signature whose P's encoding != R's bytes */

typedef signed char i8;

/* ------------------------------------------------------------------ */
/* scratch layout                                                      */
/*   tab : uint4 [nsig][FD_ATAB_STORED][8]   entry e >= 1 of signature s =*/
/*         e*(-A) in cached form, 4 canonical field elements packed    */
/*         8x32 (YpX, YmX, Z, T2d) = 128 B = one cache line, so the    */
/*         per-lane gather of a random entry moves exactly one line    */
/*   Rxy : uint4 [nsig][4]   canonical x, y of R                       */
/*   digA: i8    [64][nsig]  radix-16 signed digits of k (coalesced)   */
/*   digB: short [FD_BDIG][nsig] radix-2^FD_BWIN signed digits of S   */
/* ------------------------------------------------------------------ */

FD_DEV void fe_store_packed( uint4 * dst, fe const & a ) {
  u32 w[8]; fe_pack( w, a );
  dst[0] = make_uint4( w[0], w[1], w[2], w[3] );
  dst[1] = make_uint4( w[4], w[5], w[6], w[7] );
}
FD_DEV void fe_from_quads( fe & a, uint4 x, uint4 y ) {
  u32 w[8] = { x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w };
  fe_unpack( a, w );
}

/* entry 0 = the identity in cached form (Y+X = Y-X = Z = 1, 2dT = 0), packed
   like the stored entries: zero digits read this line instead of one per signature */
__device__ __attribute__(( aligned( 16 ) )) unsigned const fd_atab_ident_w[ 32 ] = {
  1u,0u,0u,0u, 0u,0u,0u,0u,  1u,0u,0u,0u, 0u,0u,0u,0u,  1u,0u,0u,0u, 0u,0u,0u,0u,  0u,0u,0u,0u, 0u,0u,0u,0u };

FD_DEV uint4 const * atab_entry( uint4 const * tab, u32 s, int e ) {
  return e ? tab + ((size_t)s * FD_ATAB_STORED + (size_t)( e - 1 )) * 8 : (uint4 const *)fd_atab_ident_w;
}

FD_DEV void atab_store( uint4 * tab, u32 s, int e, ge_cached const & c ) {   /* e >= 1 */
  uint4 * b = tab + ((size_t)s * FD_ATAB_STORED + (size_t)( e - 1 )) * 8;
  fe_store_packed( b + 0, c.YpX );
  fe_store_packed( b + 2, c.YmX );
  fe_store_packed( b + 4, c.Z   );
  fe_store_packed( b + 6, c.T2d );
}

struct atab_raw { uint4 q[8]; };

FD_DEV void atab_fetch( atab_raw & r, uint4 const * tab, u32 s, int e ) {
  uint4 const * b = atab_entry( tab, s, e );
#pragma unroll
  for( int i=0; i<8; i++ ) r.q[i] = b[i];
}
FD_DEV void fe_load_planar( fe & r, u32 const * p, size_t n ) {
#pragma unroll
  for( int i=0; i<10; i++ ) r.v[i] = p[(size_t)i*n];
}
FD_DEV void fe_store_planar( u32 * p, size_t n, fe const & a ) {
#pragma unroll
  for( int i=0; i<10; i++ ) p[(size_t)i*n] = a.v[i];
}
FD_DEV void fe_shfl_up( fe & r, fe const & a, int d ) {
#pragma unroll
  for( int i=0; i<10; i++ ) r.v[i] = (u32)__shfl_up( (int)a.v[i], (unsigned)d, 64 );
}
FD_DEV void fe_shfl_down( fe & r, fe const & a, int d ) {
#pragma unroll
  for( int i=0; i<10; i++ ) r.v[i] = (u32)__shfl_down( (int)a.v[i], (unsigned)d, 64 );
}

FD_DEV void atab_unpack( ge_cached & c, atab_raw const & r ) {
  fe_from_quads( c.YpX, r.q[0], r.q[1] );
  fe_from_quads( c.YmX, r.q[2], r.q[3] );
  fe_from_quads( c.Z,   r.q[4], r.q[5] );
  fe_from_quads( c.T2d, r.q[6], r.q[7] );
}

/* The order of a partitioned batch (fd_keysplit_kernel): order[] holds the nf fixed-base signatures from the front
   (none unless the context has fixed-base keys), then the nh hot ones, and the cold ones from the back;
   the decode, hash and walk kernels run one lane per place in it, in ceil(nf/256) fixed-base blocks, ceil(nh/256)
   hot blocks and then the cold blocks (at most sg + 2 in all), so a wave -- a whole block -- is of one class.
   b: the block's index among those.  cls: 2 fixed-base, 1 hot, 0 cold; j: the lane's rank in its class; col: its
   place in order[].  Returns 0 for a lane beyond its part. */
FD_DEV int ks_pos( u32 b, u32 nsig, u32 nf, u32 nh, u32 & col, u32 & j, int & cls ) {
  u32 fb = ( nf + FD_WG - 1u ) / FD_WG, hb = ( nh + FD_WG - 1u ) / FD_WG;
  cls = b < fb ? 2 : b < fb + hb ? 1 : 0;
  j = ( cls==2 ? b : cls==1 ? b - fb : b - fb - hb ) * FD_WG + threadIdx.x;
  col = cls==2 ? j : cls==1 ? nf + j : nsig - 1u - j;
  return j < ( cls==2 ? nf : cls==1 ? nh : nsig - nf - nh );
}
/* The signature at that place.  With fixed-base keys the split cannot know where the hot segment starts, so it
   lists the hot signatures in orderh[] and fd_hashh_kernel's hot lanes copy them to order[nf + j]: a kernel
   launched after the hash reads order[] alone (orderh = NULL). */
FD_DEV u32 ks_sig( u32 const * __restrict__ order, u32 const * __restrict__ orderh, u32 col, u32 j, int cls ) {
  return ( orderh && cls==1 ) ? orderh[j] : order[col];
}
/* fd_keysplit_kernel's counters (kscnt[]): hot keys, hot signatures, cold signatures, fixed-base keys claimed
   (may exceed the cap), fixed-base signatures */
#define FD_KC_HOTK 0
#define FD_KC_HOT  1
#define FD_KC_COLD 2
#define FD_KC_FBK  3
#define FD_KC_FB   4
/* ... and, past the word of the fixed-base R check's list (FD_SW_FBSLOW), the key cache's: the fixed-base
   keys of the batch found resident, those not found (the miss list's count), those that claimed a slot and build
   their tables in this batch; where the hand stood when the batch began, and the hand, which outlives the batch */
#define FD_KC_HIT   6
#define FD_KC_MISS  7
#define FD_KC_BUILD 8
#define FD_KC_HAND0 9
#define FD_KC_HAND  10
/* ... and the full slots' (DESIGN 18): the promotion tickets drawn (those below pmax list their slot in plist[]), the
   fixed-base keys whose slot is full, the signatures that walked without doublings */
#define FD_KC_PTIX  11
#define FD_KC_FFK   12
#define FD_KC_FFS   13
/* ... and the pinned keys' (DESIGN 19): the representatives whose key was found in a pinned slot, and the signatures
   that are fixed-base because of it */
#define FD_KC_PINK  14
#define FD_KC_PINS  15
/* ... and the wide tables' (DESIGN 20): the fixed-base keys whose slot was wide at the walk, and the signatures that
   walked 40 additions */
#define FD_KC_FWK   16
#define FD_KC_FWS   17

/* ------------------------------------------------------------------ */

__global__ void __launch_bounds__( FD_WG )
fd_expand_kernel( fdgpu_txn_desc_t const * __restrict__ desc, u32 txn_cnt, u32 * __restrict__ map, u32 nsig,
                  u32 * __restrict__ zero_word ) {
  u32 t = blockIdx.x * FD_WG + threadIdx.x;
  if( zero_word && t == 0u ) { zero_word[0] = 0u; zero_word[1] = 0u; }   /* the batch's slow-list count and its count
                                                                            of distinct keys (half-size path) */
  if( t >= txn_cnt ) return;
  fdgpu_txn_desc_t d = desc[t];
  for( u32 j=0; j<d.sig_cnt; j++ ) {
    u32 s = d.sig_base + j;
    if( s < nsig ) map[s] = t | (j << 24);
  }
}

/* [0..8](-A) in cached form from A's canonical affine coordinates */
template<int FM = FD_CARRY_FOLD>
FD_DEV void atab_build( uint4 * __restrict__ tab, u32 s, uint4 const * __restrict__ Axy ) {
  uint4 const * ap = Axy + (size_t)s*4;
  ge_p3 A;
  fe_from_quads( A.X, ap[0], ap[1] );
  fe_from_quads( A.Y, ap[2], ap[3] );
  A.Z = fe_one();
  fe_neg( A.X, A.X ); fe_wcarry( A.X, A.X );              /* -A */
  fe_mul<FM>( A.T, A.X, A.Y );
  ge_cached c1, c;
  ge_p3_to_cached<FM>( c1, A );
  atab_store( tab, s, 1, c1 );
  /* -A has Z = 1: each step adds it in affine form (ge_add_precomp: 3 multiplications instead of 4) */
  ge_precomp a1; a1.ypx = c1.YpX; a1.ymx = c1.YmX; a1.xy2d = c1.T2d;
  ge_p3 cur = A;
#pragma unroll 1
  for( int e=2; e<FD_ATAB_ENTRIES; e++ ) {
    ge_p1p1 tt;
    ge_add_precomp<FM>( tt, cur, a1 );
    ge_p1p1_to_p3<FM>( cur, tt );
    ge_p3_to_cached<FM>( c, cur );
    atab_store( tab, s, e, c );
  }
}

/* transaction sanity (batch size and bounds) -> ERR_SIG for all its
   signatures, like the batch_sz check of fd_ed25519_user.c:238-241 */
FD_DEV int txn_desc_ok( fdgpu_txn_desc_t const & d ) {
  u32 cnt = d.sig_cnt;
  return !( cnt==0u || cnt>16u
            || (u32)d.signature_off + 64u*cnt > (u32)d.payload_sz
            || (u32)d.acct_addr_off + 32u*cnt > (u32)d.payload_sz
            || (u32)d.message_off > (u32)d.payload_sz );
}

/* Stage 1 -- point decompression of signature s's public key A (is_r 0)
   or its R (is_r 1).  Status byte rc | small_order<<2 (rc: 0 ok, 1 not
   a square, 2 x==0 with sign set), 0xff if the transaction is
   malformed, stored at *stat; the canonical affine point goes to Axy / Rxy. */
template<int FM = FD_CARRY_FOLD>
FD_DEV void decode_one( unsigned char const * __restrict__ payload, fdgpu_txn_desc_t const * __restrict__ desc,
                        u32 const * __restrict__ map, u32 s, u32 is_r, unsigned char * __restrict__ stat,
                        uint4 * __restrict__ Rxy, uint4 * __restrict__ Axy ) {
  u32 m = map[s];
  u32 t = m & 0xffffffu, j = m >> 24;
  fdgpu_txn_desc_t d = desc[t];
  if( !txn_desc_ok( d ) ) { *stat = 0xffu; return; }
  unsigned char const * base = payload + d.payload_off;
  u32 w[8];
  fd_load_words<8>( w, base + ( is_r ? (u32)d.signature_off + 64u*j : (u32)d.acct_addr_off + 32u*j ) );
  ge_p3 P; int rc;
  ge_decode1<FM>( P, rc, w );
  int so = ge_affine_is_small_order( P );
  *stat = (unsigned char)( rc | (so << 2) );
  u32 x[8], y[8];
  fe_pack( x, P.X ); fe_pack( y, P.Y );
  uint4 * o = ( is_r ? Rxy : Axy ) + (size_t)s*4;
  o[0] = make_uint4( x[0], x[1], x[2], x[3] ); o[1] = make_uint4( x[4], x[5], x[6], x[7] );
  o[2] = make_uint4( y[0], y[1], y[2], y[3] ); o[3] = make_uint4( y[4], y[5], y[6], y[7] );
}

/* Large batches (deferred R): one lane per signature, A only.  With
   both = 1: lane 2s decodes A, lane 2s+1 R.  (No minimum waves per SIMD
   asked of the compiler: 127 VGPRs, 4 waves.) */
__global__ void __launch_bounds__( FD_WG )
fd_decode_kernel( unsigned char const *    __restrict__ payload,
                  fdgpu_txn_desc_t const * __restrict__ desc,
                  u32 const *              __restrict__ map,
                  u32                                   nsig,
                  int                                   both,
                  unsigned char *          __restrict__ pstat,
                  uint4 *                  __restrict__ Rxy,
                  uint4 *                  __restrict__ Axy,
                  uint4 *                  __restrict__ tabA,
                  uint4 *                  __restrict__ tabR,
                  u32 const *              __restrict__ ulist,
                  u32 *                    __restrict__ ucnt,
                  unsigned char *          __restrict__ astat,
                  u32                                   ublk,
                  /* fixed-base keys: the R lanes run by place in the partition, none for a
                     fixed-base signature (its R is compared undecoded); NULL: one R lane per signature */
                  u32 const *              __restrict__ order,
                  u32 const *              __restrict__ orderh,
                  u32 const *              __restrict__ kscnt,
                  /* ... and a representative whose key the context's cache held decodes nothing:
                     fidx[] names its slot, and the slot was not claimed in this batch (birth[] != batch).  Its
                     status is in astat[] already (fd_keyclass_kernel), and nothing reads its point or its -A table:
                     every signature of a fixed-base key takes the fixed-base walk */
                  u32 const *              __restrict__ kcnt,
                  u32                                   fb_min,
                  u32 const *              __restrict__ fidx,
                  u32 const *              __restrict__ birth,
                  u32                                   batch,
                  /* ... and counts the fixed-base keys whose slot is full (ucnt + 3 are the FD_KC_* words):
                     the classification and the claims are over, so full[] no longer changes in this batch */
                  u32 const *              __restrict__ full,
                  /* ... and those whose slot also has wide tables: a full slot below wcap */
                  u32                                   wcap ) {
  u32 s, is_r;
  unsigned char * st;
  if( ulist ) {
    /* keys de-duplicated (fd_keydedup_kernel): roles by block.  Blocks [0,ublk) decode A for the batch's
       representatives only -- the grid holds the worst case, blocks beyond the count on the device return at
       once -- and write A's point, status (astat, read-only from here on) and table at the representative's
       index; blocks [ublk,..) decode R for every signature */
    if( blockIdx.x < ublk ) {
      u32 i = blockIdx.x * FD_WG + threadIdx.x;
      u32 cnt = ucnt[0];
      /* for the next batch's fd_keydedup_kernel: were more than 7/8 of this one's signatures representatives?  (Of
         its sample, when this batch was not de-duplicated in full.) */
      if( !i ) {
        u32 samp = FD_KD_SBLK( ublk ) * FD_WG; samp = samp < nsig ? samp : nsig;
        ucnt[1] = ucnt[1] ? ucnt[2] > samp - ( samp >> 3 ) : cnt > nsig - ( nsig >> 3 );
        ucnt[2] = 0u;
      }
      if( i >= cnt ) return;
      s = ulist[i]; is_r = 0u; st = astat + s;
      if( fidx && kcnt[s] >= fb_min ) {
        u32 slot = fidx[s];
        if( slot != FD_FB_NONE && full[slot] ) atomicAdd( ucnt + 3 + FD_KC_FFK, 1u );
        if( slot < wcap && full[slot] ) atomicAdd( ucnt + 3 + FD_KC_FWK, 1u );   /* (FD_FB_NONE is no slot below wcap) */
        if( slot != FD_FB_NONE && birth[slot] != batch ) return;
      }
    } else if( order ) {
      u32 col, j; int cls;
      if( !ks_pos( blockIdx.x - ublk, nsig, kscnt[FD_KC_FB], kscnt[FD_KC_HOT], col, j, cls ) || cls==2 ) return;
      s = ks_sig( order, orderh, col, j, cls ); is_r = 1u;
      st = pstat + 2u*s + 1u;
    } else {
      s = ( blockIdx.x - ublk ) * FD_WG + threadIdx.x; is_r = 1u;
      if( s >= nsig ) return;
      st = pstat + 2u*s + 1u;
    }
  } else {
    u32 p = blockIdx.x * FD_WG + threadIdx.x;
    if( p >= ( both ? 2u*nsig : nsig ) ) return;
    s = both ? p >> 1 : p; is_r = both ? p & 1u : 0u;
    st = pstat + 2u*s + is_r;
  }
  decode_one( payload, desc, map, s, is_r, st, Rxy, Axy );
  /* tabA != NULL (half-size path): each lane goes on to its point's table
     when the point decoded, its table writes overlapping the other waves'
     decodes (a separate table kernel is write-heavy: 2.3 KB per signature) */
  if( tabA && ( *st & 3u )==0u ) atab_build( is_r ? tabR : tabA, s, is_r ? Rxy : Axy );
}

/* Signed digits of the base point's scalar Sw (radix 2^FD_BWIN, digB[FD_BDIG][n]) in column s.  Returns top
   raised to the highest window win( i ) at which a walk adds a nonzero digit i (the half-size walks start at
   their wave's top window). */
template<class W>
FD_DEV int store_digits_B( u32 const Sw[ 8 ], u32 s, size_t n, short * __restrict__ digB, int top, W win ) {
  int carry = 0;
#pragma unroll
  for( int i=0; i<FD_BDIG; i++ ) {
    int bit = FD_BWIN*i;
    int v = (int)((Sw[bit>>5] >> (bit&31)) & ((1u<<FD_BWIN)-1u)) + carry;
    carry = (v + (1<<(FD_BWIN-1))) >> FD_BWIN;
    int db = v - (carry << FD_BWIN);
    digB[(size_t)i*n + s] = (short)db;
    int wb = win( i );
    top = ( db && wb > top ) ? wb : top;
  }
  return top;
}

/* Signed digits of k (radix 16, digA[64][n]) and S (digB), stored coalesced. */
FD_DEV void store_digits( u32 const k[ 8 ], u32 const Sw[ 8 ], u32 s, size_t n,
                          i8 * __restrict__ digA, short * __restrict__ digB ) {
  int carry = 0;
#pragma unroll
  for( int i=0; i<64; i++ ) {
    int v = (int)((k[i>>3] >> (4*(i&7))) & 15u) + carry;
    carry = (v + 8) >> 4;
    digA[(size_t)i*n + s] = (i8)(v - (carry << 4));
  }
  (void)store_digits_B( Sw, s, n, digB, 0, []( int ) { return 0; } );   /* (the full-length walks take every window) */
}

/* ---- half-size scalars (fd_gpu_lattice.h) ------------------------------ */

/* a (5 words) x b (8 words) -> 16 words (the top 3 zero), for sc_reduce */
FD_DEV void sc_mul_5x8( u32 out[ 16 ], u32 const a[ 5 ], u32 const b[ 8 ] ) {
  u32 r[ 16 ];
#pragma unroll
  for( int i=0; i<16; i++ ) r[i] = 0u;
#pragma unroll
  for( int i=0; i<5; i++ ) {
    u64 c = 0;
#pragma unroll
    for( int j=0; j<8; j++ ) { u64 t = (u64)a[i] * (u64)b[j] + (u64)r[i+j] + c; r[i+j] = (u32)t; c = t >> 32; }
    r[i+8] = (u32)c;
  }
#pragma unroll
  for( int i=0; i<16; i++ ) out[i] = r[i];
}

/* k -> (c0, c1) with c0 == c1 k (mod 8l), re-checked here: mod 8 on the
   low words, mod l through sc_reduce (c0, |c1| k mod l < l); then
   s' = c1 S mod l.  0: no such pair within FD_LAT_BITS (full walk). */
/* HOT (a signature of a key the batch repeats): the skewed pair of fd_lat_skew, c0 of 7 words below
   2^215 (still below l, so the same comparison), |c1| below 2^79. */
template<int HOT = 0>
FD_DEV int hs_prepare( u32 const k[ 8 ], u32 const Sw[ 8 ], u32 c0[ HOT ? 7 : 5 ], u32 c1m[ 5 ], int & c1neg, u32 sp[ 8 ] ) {
  constexpr int NC = HOT ? 7 : 5;
  int ng = 0, nwin = 0;
  if( HOT ) { if( !fd_lat_skew( c0, c1m, &ng, &nwin, k ) ) return 0; }
  else if( !fd_lat_halfsize( c0, c1m, &ng, k ) ) return 0;
  c1neg = ng;
  u32 c1lo = ng ? 0u - c1m[0] : c1m[0];
  if( ( c0[0] - c1lo * k[0] ) & 7u ) return 0;                       /* mod 8 */
  u32 const lw[8] = { 0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu, 0u, 0u, 0u, 0x10000000u };
  u32 prod[ 16 ], x[ 8 ];
  sc_mul_5x8( prod, c1m, k ); sc_reduce( x, prod );                  /* |c1| k mod l */
  u32 diff = 0u;
  if( !ng ) {                                                          /* c0 == |c1| k */
#pragma unroll
    for( int i=0; i<8; i++ ) diff |= x[i] ^ ( i < NC ? c0[i] : 0u );
  } else {                                                             /* c0 + |c1| k == 0 or l */
    u64 c = 0; u32 z = 0u, e = 0u;
#pragma unroll
    for( int i=0; i<8; i++ ) {
      u64 v = (u64)x[i] + (u64)( i < NC ? c0[i] : 0u ) + c; c = v >> 32;
      z |= (u32)v; e |= (u32)v ^ lw[i];
    }
    diff = ( z != 0u ) & ( e != 0u );
  }
  if( diff ) return 0;                                                 /* mod l */
  sc_mul_5x8( prod, c1m, Sw ); sc_reduce( x, prod );                 /* |c1| S mod l */
  u32 nz = 0u;
#pragma unroll
  for( int i=0; i<8; i++ ) nz |= x[i];
  if( ng && nz ) {                                                     /* s' = l - x */
    i64 br = 0;
#pragma unroll
    for( int i=0; i<8; i++ ) { i64 t = (i64)lw[i] - (i64)x[i] + br; sp[i] = (u32)t; br = t >> 32; }
  } else {
#pragma unroll
    for( int i=0; i<8; i++ ) sp[i] = x[i];
  }
  return 1;
}

/* signed radix-16 digits of c0 and c1 (sign folded in: [c1](-R) =
   sum d_i 16^i (-R)), digA / digR [FD_HDIG][n]; s' as digB */
FD_DEV void hs_store_digits( u32 const c0[ 5 ], u32 const c1m[ 5 ], int c1neg, u32 const sp[ 8 ], u32 s, size_t n,
                             i8 * __restrict__ digA, i8 * __restrict__ digR, short * __restrict__ digB,
                             unsigned char * __restrict__ htop ) {
  int ca = 0, cr = 0, top = 0;
#pragma unroll
  for( int i=0; i<FD_HDIG; i++ ) {
    int va = (int)( ( c0[i>>3]  >> (4*(i&7)) ) & 15u ) + ca;
    int vr = (int)( ( c1m[i>>3] >> (4*(i&7)) ) & 15u ) + cr;
    /* digits in [-8,8); the top one (bits 156-159 plus the carry, <= 8 for
       values < 2^159) is kept as is: the tables hold [0..8] */
    ca = i < FD_HDIG-1 ? ( va + 8 ) >> 4 : 0; cr = i < FD_HDIG-1 ? ( vr + 8 ) >> 4 : 0;
    int dr = vr - ( cr << 4 );
    int da = va - ( ca << 4 );
    digA[(size_t)i*n + s] = (i8)da;
    digR[(size_t)i*n + s] = (i8)( c1neg ? -dr : dr );
    top = ( da | dr ) ? i : top;
  }
  /* the walks add s' digit i at window 4i (i < 8) or 4(i-8)+2 (i >= 8, the 2^120 B table): the top
     window counts these too.  (Round 4 took it from c0 / c1 alone; a wave whose pending signatures all
     had c0, c1 < 2^120 -- ~7.5e-6 of hash-distributed k, alone in a batch or in its last wave -- then
     started below window 30, skipped s' digits 7 / 15 and rejected a valid signature with ERR_MSG:
     tests/test_gpu_hs_top.py, tests/golden/hs_top.npz.) */
  top = store_digits_B( sp, s, n, digB, top, []( int i ) { return i < 8 ? 4*i : 4*(i-8) + 2; } );
  htop[s] = (unsigned char)top;                     /* highest window with a nonzero digit of c0, c1 or s' */
}

/* The window of the hot walk (fd_dsmh_kernel<.,1>) that adds s' digit j, radix 2^16: one base-point add in 16
   of the windows 0..16, never two in one, from [0..32768] (2^e B):
     j 0..4  at 4j        e = 0       j 9..12  at 4(j-9)+1   e = 140
     j 5..8  at 4(j-5)+2  e = 72      j 13..15 at 4(j-13)+3  e = 196      (16 j = 4 window + e) */
FD_DEV int hs_hot_bwin( int j ) { return j < 5 ? 4*j : j < 9 ? 4*(j-5) + 2 : j < 13 ? 4*(j-9) + 1 : 4*(j-13) + 3; }

/* Digits of a hot signature's skewed pair at column col: c0's 2 W + NW signed radix-16 digits in digA's rows
   (digit g belongs to part g / W -- [2^(68 part)](-A) -- and window g % W; the last part runs on to window
   NW - 1), c1's NW digits in digR, s' as above; htop = the highest window with a nonzero digit of any. */
FD_DEV void hs_store_digits_hot( u32 const c0[ 7 ], u32 const c1m[ 5 ], int c1neg, u32 const sp[ 8 ], u32 col, size_t n,
                                 i8 * __restrict__ digA, i8 * __restrict__ digR, short * __restrict__ digB,
                                 unsigned char * __restrict__ htop ) {
  constexpr int NA = 2*FD_KS_W + FD_KS_NW;
  int ca = 0, cr = 0, top = 0;
  /* a word of c0 per round, not 54 unrolled digits: unrolled, their values and addresses stay live together
     and cost the hash kernel its third wave (193 VGPRs against 167) */
  u32 cw[ 7 ];
#pragma unroll
  for( int i=0; i<7; i++ ) cw[i] = c0[i];
  i8 * pa = digA + col;
#pragma unroll 1
  for( int wd=0; wd<7; wd++ ) {
    u32 x = cw[0];
#pragma unroll
    for( int i=0; i<6; i++ ) cw[i] = cw[i+1];
#pragma unroll
    for( int j=0; j<8; j++ ) {
      int i = 8*wd + j;
      if( i < NA ) {
        int va = (int)( ( x >> (4*j) ) & 15u ) + ca;
        ca = i < NA-1 ? ( va + 8 ) >> 4 : 0;        /* (c0 < 2^215: the top digit, kept as is, is <= 8) */
        int da = va - ( ca << 4 );
        *pa = (i8)da; pa += n;
        int w = i < FD_KS_W ? i : i < 2*FD_KS_W ? i - FD_KS_W : i - 2*FD_KS_W;
        top = ( da && w > top ) ? w : top;
      }
    }
  }
#pragma unroll
  for( int i=0; i<FD_KS_NW; i++ ) {
    int vr = (int)( ( c1m[i>>3] >> (4*(i&7)) ) & 15u ) + cr;
    cr = i < FD_KS_NW-1 ? ( vr + 8 ) >> 4 : 0;      /* (|c1| < 2^79) */
    int dr = vr - ( cr << 4 );
    digR[(size_t)i*n + col] = (i8)( c1neg ? -dr : dr );
    top = ( dr && i > top ) ? i : top;
  }
  /* (store_digits_B's loop, written out: through the shared copy fd_hashh_kernel<1> compiles differently) */
  int carry = 0;
#pragma unroll
  for( int i=0; i<FD_BDIG; i++ ) {
    int bit = FD_BWIN*i;
    int v = (int)((sp[bit>>5] >> (bit&31)) & ((1u<<FD_BWIN)-1u)) + carry;
    carry = (v + (1<<(FD_BWIN-1))) >> FD_BWIN;
    int db = v - (carry << FD_BWIN);
    digB[(size_t)i*n + col] = (short)db;
    int wb = hs_hot_bwin( i );                      /* htop counts the base-point windows too (test_gpu_hs_top.py) */
    top = ( db && wb > top ) ? wb : top;
  }
  htop[col] = (unsigned char)top;
}

/* The wave's top window (half-size walks): the largest htop of its pending
   signatures, every lane of the wave still active */
FD_DEV int hs_wave_top( int pend, unsigned char const * __restrict__ htop, u32 s ) {
  int wtop = pend ? (int)htop[s] : 0;
#pragma unroll
  for( int o=32; o>0; o>>=1 ) { int v = __shfl_xor( wtop, o, 64 ); wtop = v > wtop ? v : wtop; }
  return wtop;
}

/* The result-code procedure of fd_ed25519_verify (fd_ed25519_user.c:
   174-199) from S's check (code so far: SUCCESS or
   ERR_SIG) and the point statuses pa (A) and pr (R).  defer: R has not
   been decoded (pr = 0); a small-order A is parked as FD_PEND_ASMALL,
   because its code depends on whether R decodes (check 3 comes before
   check 4). */
FD_DEV int result_code( int code, u32 pa, u32 pr, int semantics, int defer ) {
  if( pa==0xffu || pr==0xffu ) return FD_ED25519_ERR_SIG;                    /* malformed transaction */
  if( code != FD_ED25519_SUCCESS ) return code;                             /* (1) S < l */
  int ra = (int)(pa & 3u), rb = (int)(pr & 3u);
  if( semantics==FDGPU_SEMANTICS_AVX512 ) {
    if( ra | rb ) return FD_ED25519_ERR_SIG;                                /* (2)(3) decode (AVX-512) */
  } else {
    if( ra==1 ) return FD_ED25519_ERR_PUBKEY;                               /* (2) decode (portable) */
    if( rb==1 ) return FD_ED25519_ERR_SIG;                                  /* (3) */
  }
  if( pa & 4u ) return defer ? FD_PEND_ASMALL : FD_ED25519_ERR_PUBKEY;      /* (4) small-order A */
  if( pr & 4u ) return FD_ED25519_ERR_SIG;                                  /* (5) small-order R */
  return FD_ED25519_SUCCESS;
}

/* Stage 2 -- S's check and k = SHA-512(R||A||M) mod l (:204-206) with
   the signed digits of k and S.
   defer = 1 (large batches): after the decode of A; sets the code from
   pstat and hashes only pending signatures; keeps R's bytes for the
   R-check kernels.
   defer = 0, statuses = 0 (small batches, fd_prep_kernel): runs beside
   the decodes; writes ERR_SIG (malformed or S >= l) or SUCCESS and
   hashes every well-formed signature; fd_table_kernel applies the
   point statuses. */
/* The front of every hash role (hash_one, hashh_one, hashh_one_q): signature s's transaction descriptor d and
   its signer j; 0 if the descriptor is malformed.  (Only this much is shared: with S's load and check in
   here too, every hash kernel compiles differently.) */
FD_DEV int sig_desc( fdgpu_txn_desc_t const * __restrict__ desc, u32 const * __restrict__ map, u32 s,
                     fdgpu_txn_desc_t & d, u32 & j ) {
  u32 m = map[s];
  u32 t = m & 0xffffffu;
  j = m >> 24;
  d = desc[t];
  return txn_desc_ok( d );
}

/* h = signature s's SHA-512(R||A||M), computed beforehand (messages beyond the descriptor range, verify_long) */
FD_DEV void khash_load( u32 h[ 16 ], uint4 const * __restrict__ khash, u32 s ) {
#pragma unroll
  for( int i=0; i<4; i++ ) { uint4 v = khash[4*(size_t)s + i]; h[4*i] = v.x; h[4*i+1] = v.y; h[4*i+2] = v.z; h[4*i+3] = v.w; }
}

FD_DEV void hash_one( unsigned char const * __restrict__ payload, fdgpu_txn_desc_t const * __restrict__ desc,
                      u32 const * __restrict__ map, u32 s, size_t n, int semantics, int defer,
                      unsigned char const * __restrict__ pstat, i8 * __restrict__ code_out,
                      i8 * __restrict__ digA, short * __restrict__ digB, uint4 * __restrict__ Rraw,
                      uint4 const * __restrict__ khash ) {
  fdgpu_txn_desc_t d; u32 j;
  if( !sig_desc( desc, map, s, d, j ) ) { code_out[s] = FD_ED25519_ERR_SIG; return; }
  unsigned char const * base = payload + d.payload_off;
  u32 Sw[8];
  fd_load_words<8>( Sw, base + d.signature_off + 64u*j + 32u );
  int code = sc_is_canonical( Sw ) ? FD_ED25519_SUCCESS : FD_ED25519_ERR_SIG;
  if( defer ) code = result_code( code, pstat[2*s], 0u, semantics, 1 );
  code_out[s] = (i8)code;
  if( code != FD_ED25519_SUCCESS && code != FD_PEND_ASMALL ) return;

  u32 Rw[8], Aw[8];
  fd_load_words<8>( Rw, base + d.signature_off + 64u*j );
  if( defer ) {
    Rraw[2*(size_t)s]   = make_uint4( Rw[0], Rw[1], Rw[2], Rw[3] );        /* R's bytes for the R-check kernels */
    Rraw[2*(size_t)s+1] = make_uint4( Rw[4], Rw[5], Rw[6], Rw[7] );
    if( code != FD_ED25519_SUCCESS ) return;
  }
  fd_load_words<8>( Aw, base + d.acct_addr_off + 32u*j );
  u32 h[16], k[8];
  if( khash ) khash_load( h, khash, s );
  else fd_sha512_RAM( h, Rw, Aw, base + d.message_off, (u32)d.payload_sz - (u32)d.message_off );
  sc_reduce( k, h );
  store_digits( k, Sw, s, n, digA, digB );
}

__global__ void __launch_bounds__( FD_WG )
fd_hash_kernel( unsigned char const *    __restrict__ payload,
                fdgpu_txn_desc_t const * __restrict__ desc,
                u32 const *              __restrict__ map,
                u32                                   nsig,
                int                                   semantics,
                int                                   defer,
                unsigned char const *    __restrict__ pstat,
                i8 *                     __restrict__ code_out,
                i8 *                     __restrict__ digA,
                short *                  __restrict__ digB,
                uint4 *                  __restrict__ Rraw,
                uint4 const *            __restrict__ khash ) {
  u32 s = blockIdx.x * FD_WG + threadIdx.x;
  if( s >= nsig ) return;
  if( !defer ) {                                 /* both points decoded already */
    hash_one( payload, desc, map, s, nsig, semantics, 0, pstat, code_out, digA, digB, Rraw, khash );
    int c = code_out[s];
    if( c==FD_ED25519_SUCCESS || c==FD_ED25519_ERR_SIG )
      code_out[s] = (i8)result_code( c, pstat[2*s], pstat[2*s+1], semantics, 0 );
    return;
  }
  hash_one( payload, desc, map, s, nsig, semantics, 1, pstat, code_out, digA, digB, Rraw, khash );
}

/* Half-size path, after the decode of A and R: the full result-code
   procedure, then for the signatures still pending k = SHA-512(R||A||M)
   mod l, the reduction to (c0, c1) and s' = c1 S mod l, stored as digits.
   A signature without a short pair keeps the digits of k and S and goes
   on the slow list (FD_PEND_SLOW). */
/* rc = 1 (throughput, after both decodes): the full result-code procedure
   first, and a slow signature is flagged in pstat; rc = 0 (fd_prep_kernel,
   beside the decodes): S's check only -- the DSM applies the rest. */
/* KS (the batch partitioned into hot and cold signatures, fd_keysplit_kernel): digits, htop and the slow list's
   entry go to column col, the signature's place in that order; a hot one (block-uniform) gets the skewed pair. */
template<int KS = 0>
FD_DEV void hashh_one( unsigned char const * __restrict__ payload, fdgpu_txn_desc_t const * __restrict__ desc,
                       u32 const * __restrict__ map, u32 s, size_t n, int semantics, int rc,
                       unsigned char * __restrict__ pstat, i8 * __restrict__ code_out, i8 * __restrict__ digA,
                       i8 * __restrict__ digR, short * __restrict__ digB, u32 * __restrict__ slow,
                       u32 * __restrict__ slow_cnt, uint4 const * __restrict__ khash, u32 force_slow,
                       unsigned char * __restrict__ htop, u32 const * __restrict__ arep = (u32 const *)0,
                       unsigned char const * __restrict__ astat = (unsigned char const *)0, u32 kcol = 0u, int hot = 0 ) {
  u32 col = KS ? kcol : s;
  fdgpu_txn_desc_t d; u32 j;
  if( !sig_desc( desc, map, s, d, j ) ) { code_out[s] = FD_ED25519_ERR_SIG; return; }
  unsigned char const * base = payload + d.payload_off;
  u32 Sw[8];
  fd_load_words<8>( Sw, base + d.signature_off + 64u*j + 32u );
  int code = sc_is_canonical( Sw ) ? FD_ED25519_SUCCESS : FD_ED25519_ERR_SIG;
  /* arep (keys de-duplicated): A's status is the representative's, in an array nothing writes after the
     decode -- pstat[2s] then holds only this signature's own FD_PSTAT_SLOW flag, which a representative's
     lane may set while another signature of its key reads A's status */
  if( rc ) code = result_code( code, arep ? astat[ arep[s] ] : pstat[2*s], pstat[2*s+1], semantics, 0 );
  if( code != FD_ED25519_SUCCESS ) { code_out[s] = (i8)code; return; }
  u32 Rw[8], Aw[8];
  fd_load_words<8>( Rw, base + d.signature_off + 64u*j );
  fd_load_words<8>( Aw, base + d.acct_addr_off + 32u*j );
  u32 h[16], k[8];
  if( khash ) khash_load( h, khash, s );
  else fd_sha512_RAM( h, Rw, Aw, base + d.message_off, (u32)d.payload_sz - (u32)d.message_off );
  sc_reduce( k, h );
  u32 c0[5], c1m[5], sp[8]; int c1neg = 0;
  if( KS && hot ) {
    u32 c0h[7];
    if( !( force_slow && s % force_slow == 0u ) && hs_prepare<1>( k, Sw, c0h, c1m, c1neg, sp ) ) {
      hs_store_digits_hot( c0h, c1m, c1neg, sp, col, n, digA, digR, digB, htop );
      code_out[s] = FD_ED25519_SUCCESS;
      return;
    }
  } else if( !( force_slow && s % force_slow == 0u ) && hs_prepare( k, Sw, c0, c1m, c1neg, sp ) ) {
    hs_store_digits( c0, c1m, c1neg, sp, col, n, digA, digR, digB, htop );
    code_out[s] = FD_ED25519_SUCCESS;
    return;
  }
  store_digits( k, Sw, col, n, digA, digB );
  code_out[s] = FD_PEND_SLOW;
  if( rc ) pstat[2*s] |= FD_PSTAT_SLOW;            /* fd_dsmh_kernel's half-size blocks skip it even once its code is final */
  slow[ atomicAdd( slow_cnt, 1u ) ] = col;
}

/* The latency path's hash role on a quad of lanes (fd_prep_kernel<.,1,1>): the S check and the loads on all
   four, SHA-512 shared (fd_sha512_RAM_quad), then lane q = 0 alone goes on as hashh_one does (rc = 0: S's
   check only; the DSM applies the rest).  Every exit before the digest is the quad's together. */
FD_DEV void hashh_one_q( unsigned char const * __restrict__ payload, fdgpu_txn_desc_t const * __restrict__ desc,
                         u32 const * __restrict__ map, u32 s, size_t n, i8 * __restrict__ code_out,
                         i8 * __restrict__ digA, i8 * __restrict__ digR, short * __restrict__ digB,
                         u32 * __restrict__ slow, u32 * __restrict__ slow_cnt, uint4 const * __restrict__ khash,
                         u32 force_slow, unsigned char * __restrict__ htop, u32 q, u32 qbase ) {
  fdgpu_txn_desc_t d; u32 j;
  if( !sig_desc( desc, map, s, d, j ) ) { if( !q ) code_out[s] = FD_ED25519_ERR_SIG; return; }
  unsigned char const * base = payload + d.payload_off;
  u32 Sw[8];
  fd_load_words<8>( Sw, base + d.signature_off + 64u*j + 32u );
  if( !sc_is_canonical( Sw ) ) { if( !q ) code_out[s] = FD_ED25519_ERR_SIG; return; }
  u32 Rw[8], Aw[8];
  fd_load_words<8>( Rw, base + d.signature_off + 64u*j );
  fd_load_words<8>( Aw, base + d.acct_addr_off + 32u*j );
  u32 h[16], k[8];
  if( khash ) {                                  /* digests computed before (long messages): lane 0 reads its own */
    if( q ) return;
    khash_load( h, khash, s );
  } else {
    fd_sha512_RAM_quad( h, Rw, Aw, base + d.message_off, (u32)d.payload_sz - (u32)d.message_off, q, qbase );
    if( q ) return;
  }
  sc_reduce( k, h );
  u32 c0[5], c1m[5], sp[8]; int c1neg = 0;
  if( !( force_slow && s % force_slow == 0u ) && hs_prepare( k, Sw, c0, c1m, c1neg, sp ) ) {
    hs_store_digits( c0, c1m, c1neg, sp, s, n, digA, digR, digB, htop );
    code_out[s] = FD_ED25519_SUCCESS;
  } else {
    store_digits( k, Sw, s, n, digA, digB );
    code_out[s] = FD_PEND_SLOW;
    slow[ atomicAdd( slow_cnt, 1u ) ] = s;
  }
}

/* The high tables of hot key number hi: [1..8]( [2^(68 (part+1))](-A) ) in the -A table's entry format, at table
   index 2 hi + part of htab, from the representative's canonical affine A */
template<int FM = FD_CARRY_FOLD>
FD_DEV void htab_build( uint4 * __restrict__ htab, u32 hi, u32 part, uint4 const * __restrict__ Axy, u32 rep ) {
  uint4 const * ap = Axy + (size_t)rep*4;
  ge_p3 A;
  fe_from_quads( A.X, ap[0], ap[1] );
  fe_from_quads( A.Y, ap[2], ap[3] );
  A.Z = fe_one();
  fe_neg( A.X, A.X ); fe_wcarry( A.X, A.X );              /* -A */
  fe_mul<FM>( A.T, A.X, A.Y );
  int nd = 4*FD_KS_W*( (int)part + 1 );
#pragma unroll 1
  for( int i=0; i<nd; i++ ) ge_p3_dbl<FM>( A, A );
  u32 t = 2u*hi + part;
  ge_cached c1;
  ge_p3_to_cached<FM>( c1, A );
  atab_store( htab, t, 1, c1 );
#pragma unroll 1
  for( int e=2; e<FD_ATAB_ENTRIES; e++ ) {
    ge_p1p1 tt;
    ge_add_cached<FM>( tt, A, c1 );
    ge_p1p1_to_p3<FM>( A, tt );
    /* the entry stored one element at a time: a whole ge_cached beside A, c1 and the sum costs the hash
       kernel its third wave */
    uint4 * b = htab + ((size_t)t * FD_ATAB_STORED + (size_t)( e - 1 )) * 8;
    fe u;
    fe_add( u, A.Y, A.X ); fe_store_packed( b + 0, u );
    fe_sub( u, A.Y, A.X ); fe_store_packed( b + 2, u );
    fe_store_packed( b + 4, A.Z );
    fe d2 = fe_d2(); fe_mul<FM>( u, A.T, d2 ); fe_store_packed( b + 6, u );
  }
}

/* ---- fixed-base keys ------------------------------------------
   A key with FD_FB_MIN signatures in a batch is treated like the base point: its signatures are verified as
     P = [S]B + [k](-A),  k = sum_{j<32} a_j 2^(8j),  S = sum_{i<16} b_i 2^(16i)   (signed digits)
   from FD_FB_T tables per key, T_t = { [e]( [2^(32t)](-A) ) : e = 1..FD_FB_E }, and the base point's
   [0..32768]( [2^(32t)]B ), in 24 doublings, and P's encoding is compared with R's 32 bytes by the full-length
   path's R-check kernels: no lattice reduction, no decode of R, no -R table. */

/* Hash role of a fixed-base signature at place col: the result code with R's check deferred (hash_one with
   defer = 1: a small-order A parked as FD_PEND_ASMALL), R's bytes to Rraw[4 s] (the signature's own, unused Rxy
   slot), the 32 signed radix-256 digits of k mod l to digA's rows [0, 32) and S's 16 digits to digB */
FD_DEV void hashf_one( unsigned char const * __restrict__ payload, fdgpu_txn_desc_t const * __restrict__ desc,
                       u32 const * __restrict__ map, u32 s, size_t n, int semantics, u32 pa,
                       i8 * __restrict__ code_out, i8 * __restrict__ digA, short * __restrict__ digB,
                       uint4 * __restrict__ Rraw, uint4 const * __restrict__ khash, u32 col ) {
  fdgpu_txn_desc_t d; u32 j;
  if( !sig_desc( desc, map, s, d, j ) ) { code_out[s] = FD_ED25519_ERR_SIG; return; }
  unsigned char const * base = payload + d.payload_off;
  u32 Sw[8];
  fd_load_words<8>( Sw, base + d.signature_off + 64u*j + 32u );
  int code = sc_is_canonical( Sw ) ? FD_ED25519_SUCCESS : FD_ED25519_ERR_SIG;
  code = result_code( code, pa, 0u, semantics, 1 );
  code_out[s] = (i8)code;
  if( code != FD_ED25519_SUCCESS && code != FD_PEND_ASMALL ) return;
  u32 Rw[8], Aw[8];
  fd_load_words<8>( Rw, base + d.signature_off + 64u*j );
  Rraw[4*(size_t)s]   = make_uint4( Rw[0], Rw[1], Rw[2], Rw[3] );
  Rraw[4*(size_t)s+1] = make_uint4( Rw[4], Rw[5], Rw[6], Rw[7] );
  if( code != FD_ED25519_SUCCESS ) return;
  fd_load_words<8>( Aw, base + d.acct_addr_off + 32u*j );
  u32 h[16], k[8];
  if( khash ) khash_load( h, khash, s );
  else fd_sha512_RAM( h, Rw, Aw, base + d.message_off, (u32)d.payload_sz - (u32)d.message_off );
  sc_reduce( k, h );
  i8 dk[ 32 ];
  (void)fd_fb_recode( dk, k );                       /* (k < l: no carry out of the top digit) */
#pragma unroll
  for( int i=0; i<32; i++ ) digA[(size_t)i*n + col] = dk[i];
  (void)store_digits_B( Sw, col, n, digB, 0, []( int ) { return 0; } );
}

/* P_j = [2^(8j)](-A) of the key in slot fi in the -A table's entry format at fbase[32 fi + j]: A doubled nd times.  A
   claim runs one lane per (key, t) with j = 4t from the representative's canonical affine A (fbase_build), so the
   chain of up to 224 doublings is paid by 8 lanes of a key and not by the 1,024 that build its entries. */
template<int FM = FD_CARRY_FOLD>
FD_DEV void chain_store( uint4 * __restrict__ b, ge_p3 & A, int nd ) {
#pragma unroll 1
  for( int i=0; i<nd; i++ ) ge_p3_dbl<FM>( A, A );
  ge_cached c;
  ge_p3_to_cached<FM>( c, A );
  fe_store_packed( b + 0, c.YpX );
  fe_store_packed( b + 2, c.YmX );
  fe_store_packed( b + 4, c.Z   );
  fe_store_packed( b + 6, c.T2d );
}
template<int FM = FD_CARRY_FOLD>
FD_DEV void fbase_chain( uint4 * __restrict__ fbase, u32 fi, u32 j, ge_p3 & A, int nd ) {
  chain_store<FM>( fbase + ( (size_t)fi * FD_FB_NT + j ) * 8, A, nd );
}
/* (2X : 2Y : 2Z) of the point a cached entry (Y+X, Y-X, Z, 2dT) holds: all a doubling reads (no T) */
FD_DEV void cached_to_dbl_input( ge_p3 & A, uint4 const * __restrict__ e ) {
  fe ypx, ymx;
  fe_from_quads( ypx, e[0], e[1] ); fe_from_quads( ymx, e[2], e[3] ); fe_from_quads( A.Z, e[4], e[5] );
  fe_sub( A.X, ypx, ymx ); fe_wcarry( A.X, A.X );
  fe_add( A.Y, ypx, ymx ); fe_wcarry( A.Y, A.Y );
  fe_add( A.Z, A.Z, A.Z ); fe_wcarry( A.Z, A.Z ); A.T = fe_zero();
}
/* Wide tables: the 16 extra base points of slot fi, wbase[( 8 fi + t ) 2 + r - 1] = [2^(32t + 11r)](-A) for
   r = 1, 2, by 11 r doublings from the slot's own P_4t; lane q = 2t + r - 1 of the slot's 16 */
FD_DEV void wbase_chain( uint4 * __restrict__ wbase, uint4 const * __restrict__ fbase, u32 fi, u32 q ) {
  u32 t = q >> 1, r = ( q & 1u ) + 1u;
  ge_p3 A;
  cached_to_dbl_input( A, fbase + ( (size_t)fi * FD_FB_NT + 4u*t ) * 8 );
  chain_store( wbase + ( (size_t)fi * 16u + q ) * 8, A, 11*(int)r );
}
template<int FM = FD_CARRY_FOLD>
FD_DEV void fbase_build( uint4 * __restrict__ fbase, u32 fi, u32 j, uint4 const * __restrict__ Axy, u32 rep ) {
  uint4 const * ap = Axy + (size_t)rep*4;
  ge_p3 A;
  fe_from_quads( A.X, ap[0], ap[1] );
  fe_from_quads( A.Y, ap[2], ap[3] );
  A.Z = fe_one();
  fe_neg( A.X, A.X ); fe_wcarry( A.X, A.X );              /* -A */
  fe_mul<FM>( A.T, A.X, A.Y );
  fbase_chain<FM>( fbase, fi, j, A, 8*(int)j );
}

/* the identity in affine precomputed form (y+x = y-x = 1, 2dxy = 0), packed like a table entry: digit 0 */
__device__ __attribute__(( aligned( 16 ) )) unsigned const fd_ptab_ident_w[ 24 ] = {
  1u,0u,0u,0u, 0u,0u,0u,0u,  1u,0u,0u,0u, 0u,0u,0u,0u,  0u,0u,0u,0u, 0u,0u,0u,0u };
/* (the host's copy: the head of the wide tables' array) */
static unsigned const fd_ptab_ident_host[ 24 ] = {
  1u,0u,0u,0u, 0u,0u,0u,0u,  1u,0u,0u,0u, 0u,0u,0u,0u,  0u,0u,0u,0u, 0u,0u,0u,0u };

/* entry e >= 1 of table j (of FD_FB_NT) of the key in slot fi: 6 uint4 (ypx, ymx, xy2d, canonical, packed 8x32) */
FD_DEV size_t ftab_at( u32 fi, u32 j, u32 e ) {
  return ( ( (size_t)fi * FD_FB_NT + j ) * FD_FB_E + ( e - 1u ) ) * 6;
}
/* entry e >= 1 of wide table (t, r) of the key in slot fi, in the same format.  wtab[] begins with the
   identity entry, so a zero digit reads offset 0 of the same array and the walk's gathers need no second base */
FD_DEV size_t wtab_at( u32 fi, u32 t, u32 r, u32 e ) {
  return ( ( (size_t)fi * 8u * FD_FB_WE + (size_t)fd_fb_wide_off( (int)t, (int)r ) ) + e ) * 6;
}

/* fd_ftab_kernel's two passes over a lane's eight points, written as recursions over the point's number so
   that every index of the prefix array pf[] is a constant and the array stays in registers.
   Pass 1, point I: Q += P_t, parked projective in its own entry (X, Y, Z: 96 B); pf[I] = Z_0 ... Z_I. */
template<int I>
FD_DEV void ftab_pass1( ge_p3 & Q, ge_cached const & pc, uint4 * __restrict__ ent, fe (&pf)[ 8 ] ) {
  ge_p1p1 tt;
  ge_add_cached( tt, Q, pc ); ge_p1p1_to_p3( Q, tt );
  fe_store_packed( ent + 6*I + 0, Q.X );
  fe_store_packed( ent + 6*I + 2, Q.Y );
  fe_store_packed( ent + 6*I + 4, Q.Z );
  if constexpr( I > 0 ) fe_mul( pf[I], pf[I-1], Q.Z ); else pf[0] = Q.Z;
  if constexpr( I < 7 ) ftab_pass1<I+1>( Q, pc, ent, pf );
}
/* Pass 2, from point 7 down, inv = 1 / (Z_0 ... Z_I) on entry: 1/Z_I = inv pf[I-1], then the affine precomputed
   entry (y+x, y-x, 2dxy) over the parked point */
template<int I>
FD_DEV void ftab_pass2( fe & inv, uint4 * __restrict__ ent, fe const (&pf)[ 8 ] ) {
  fe X, Y, Z, zi, x, y, u;
  fe_from_quads( X, ent[6*I+0], ent[6*I+1] );
  fe_from_quads( Y, ent[6*I+2], ent[6*I+3] );
  if constexpr( I > 0 ) {
    fe_from_quads( Z, ent[6*I+4], ent[6*I+5] );
    fe_mul( zi, inv, pf[I-1] ); fe_mul( inv, inv, Z );
  } else zi = inv;
  fe_mul( x, X, zi ); fe_mul( y, Y, zi );
  fe_add( u, y, x ); fe_store_packed( ent + 6*I + 0, u );
  fe_sub( u, y, x ); fe_store_packed( ent + 6*I + 2, u );
  fe d2 = fe_d2();
  fe_mul( u, x, y ); fe_mul( u, u, d2 ); fe_store_packed( ent + 6*I + 4, u );
  if constexpr( I > 0 ) ftab_pass2<I-1>( inv, ent, pf );
}

/* The entries of the fixed-base keys' tables: 128 lanes per work item (slot, group r) -- a workgroup holds two
   items -- lane (t, g) with g = 0..15 builds entries 8g + 1 .. 8g + 8 of the slot's table j = 4t + r (a claim lists
   group 0, a promotion groups 1..3: DESIGN 18).  It starts at [8g]P_j by double-and-add over g's 4 bits
   and three doublings, adds P_j eight times, and normalises its eight points with Montgomery's trick: the
   product of its own eight Z, the products of the other lanes' through lane-shuffle prefix and suffix products
   as in fd_rprod_kernel, one inversion per wave (every lane computes it: no lane of the wave has anything else
   to do), then 1/Z_i = (prefix of the lane's Z below i) x (running inverse).  Blocks beyond the device-side count
   of fixed-base keys return at once; a key that does not decode or has small order has no table (its
   signatures' codes are final or parked before any walk). */
__global__ void __launch_bounds__( FD_WG, 2 )          /* (two waves per SIMD asked for: the eight prefix products are 80 VGPRs) */
fd_ftab_kernel( u32 const * __restrict__ kscnt, u32 const * __restrict__ flist,
                unsigned char const * __restrict__ astat, uint4 const * __restrict__ fbase, uint4 * __restrict__ ftab,
                /* a work item is (slot, group r), the 8 tables j = 4t + r of the slot.  Items [0, cg nk)
                   are the claims' groups 0..cg-1 (cg = 1; 4 with fdgpu_debug_opts_t.key_full = 2); the items after
                   them are groups 1..3 of the slots promoted in this batch (plist[], at most pmax) */
                u32 cg, u32 const * __restrict__ plist, u32 pmax,
                /* behind those, the wide tables of the slots below wcap: 24 items a slot, item q = 3t + r
                   being the 128 lanes of wide table (t, r), lane g building entries 8g + 1 .. 8g + 8 -- first of the
                   claims' slots when a claim fills its slot at once (wnow), then of the promoted slots' */
                uint4 const * __restrict__ wbase, uint4 * __restrict__ wtab, u32 wcap, u32 wnow ) {
  u32 nk = kscnt[FD_KC_BUILD] * cg;                       /* the keys that claimed a slot in this batch */
  u32 np = kscnt[FD_KC_PTIX]; np = np < pmax ? np : pmax;
  u32 nb = nk + 3u*np;                                    /* the items of the byte tables */
  u32 nkw = wcap && wnow ? kscnt[FD_KC_BUILD] * 24u : 0u, nw = wcap ? nkw + 24u*np : 0u;
  u32 bi = blockIdx.x * 2u + ( threadIdx.x >> 7 );
  if( blockIdx.x * 2u >= nb + nw ) return;                /* (block-uniform) */
  /* a wave is of one item: lanes of an item that is beyond the count, or of a key without tables, skip the work
     together */
  if( bi >= nb + nw ) return;
  u32 fi, grp, t, g;
  int top = 3;                                            /* the highest bit of g */
  uint4 const * bp; uint4 * ent;
  if( bi < nb ) {
    if( bi < nk ) {
      if( astat[ flist[ 2u*( bi / cg ) + 1u ] ] & 7u ) return;
      fi = flist[ 2u*( bi / cg ) ]; grp = bi % cg;        /* its slot */
    } else { fi = plist[ ( bi - nk ) / 3u ]; grp = ( bi - nk ) % 3u + 1u; }   /* (promoted: the slot has tables) */
    t = 4u*( ( threadIdx.x >> 4 ) & 7u ) + grp; g = threadIdx.x & 15u;
    bp = fbase + ( (size_t)fi * FD_FB_NT + t ) * 8;
    ent = ftab + ftab_at( fi, t, 8u*g + 1u );
  } else {
    u32 wi = bi - nb, q;
    if( wi < nkw ) {
      if( astat[ flist[ 2u*( wi / 24u ) + 1u ] ] & 7u ) return;
      fi = flist[ 2u*( wi / 24u ) ]; q = wi % 24u;
    } else { fi = plist[ ( wi - nkw ) / 24u ]; q = ( wi - nkw ) % 24u; }
    if( fi >= wcap ) return;                              /* (a slot without wide tables) */
    t = q / 3u; u32 r = q % 3u;
    /* a table of fewer than 1,024 entries: the lanes beyond it repeat its last lane's work, in step with it and
       with the same values to the same addresses (they are lanes of the last lane's own wave: the tables' sizes are
       multiples of 8 and the wave's first lane is always inside), so the wave's shuffles need no special case */
    g = threadIdx.x & 127u;
    u32 gl = (u32)fd_fb_wide_entries( (int)r ) / 8u - 1u; g = g < gl ? g : gl;
    top = 6;
    bp = r ? wbase + ( (size_t)fi * 16u + 2u*t + r - 1u ) * 8 : fbase + ( (size_t)fi * FD_FB_NT + 4u*t ) * 8;
    ent = wtab + wtab_at( fi, t, r, 8u*g + 1u );
  }
  int lane = (int)( threadIdx.x & 63u );
  ge_cached pc;
  {
    atab_raw r;
#pragma unroll
    for( int i=0; i<8; i++ ) r.q[i] = bp[i];
    atab_unpack( pc, r );
  }
  ge_p3 Q; ge_p3_identity( Q );
  ge_p1p1 tt;
#pragma unroll 1
  for( int b=top; b>=0; b-- ) {                           /* [g]P_t */
    ge_p3_dbl( Q, Q );
    ge_add_cached( tt, Q, pc );
    ge_p3 Qa; ge_p1p1_to_p3( Qa, tt );
    int bit = (int)( ( g >> b ) & 1u );
    fe_sel( Q.X, bit, Qa.X, Q.X ); fe_sel( Q.Y, bit, Qa.Y, Q.Y ); fe_sel( Q.Z, bit, Qa.Z, Q.Z ); fe_sel( Q.T, bit, Qa.T, Q.T );
  }
#pragma unroll 1
  for( int b=0; b<3; b++ ) ge_p3_dbl( Q, Q );             /* [8g]P_t */
  /* pass 1: the eight points, projective, parked in their own entries (X, Y, Z: 96 B), and the prefix products
     of their Z */
  fe pf[ 8 ];
  ftab_pass1<0>( Q, pc, ent, pf );
  /* the inverse of the lane's product: the wave's prefix and suffix products of the lanes' products, the wave's
     total inverted, times the other lanes' product */
  fe one = fe_one(), pre = pf[7], suf = pf[7], u;
#pragma unroll 1
  for( int d=1; d<64; d<<=1 ) {
    fe_shfl_up( u, pre, d );   fe_sel( u, lane >= d, u, one );     fe_mul( pre, pre, u );
    fe_shfl_down( u, suf, d ); fe_sel( u, lane + d < 64, u, one ); fe_mul( suf, suf, u );
  }
  fe o, e, tot, inv;
  fe_shfl_up( o, pre, 1 );   fe_sel( o, lane > 0, o, one );
  fe_shfl_down( e, suf, 1 ); fe_sel( e, lane < 63, e, one );
  fe_mul( o, o, e );                                      /* the other lanes' product */
#pragma unroll
  for( int i=0; i<10; i++ ) tot.v[i] = (u32)__shfl( (int)pre.v[i], 63, 64 );
  fe_invert( inv, tot );
  fe_mul( inv, inv, o );                                  /* 1 / (Z_1 ... Z_8) of this lane */
  /* pass 2, from the last point down: 1/Z_i, then the affine precomputed entry over the parked point */
  ftab_pass2<7>( inv, ent, pf );
}

/* (no minimum waves per SIMD asked of the compiler: the lattice reduction sets 159 VGPRs, 3 waves) */
template<int KS>
__global__ void __launch_bounds__( FD_WG )
fd_hashh_kernel( unsigned char const *    __restrict__ payload,
                 fdgpu_txn_desc_t const * __restrict__ desc,
                 u32 const *              __restrict__ map,
                 u32                                   nsig,
                 int                                   semantics,
                 unsigned char *          __restrict__ pstat,
                 i8 *                     __restrict__ code_out,
                 i8 *                     __restrict__ digA,
                 i8 *                     __restrict__ digR,
                 short *                  __restrict__ digB,
                 u32 *                    __restrict__ slow,
                 u32 *                    __restrict__ slow_cnt,
                 uint4 const *            __restrict__ khash,
                 u32                                   force_slow,
                 unsigned char *          __restrict__ htop,
                 u32 const *              __restrict__ arep,
                 unsigned char const *    __restrict__ astat,
                 /* KS (hot / cold partition, fd_keysplit_kernel): */
                 u32 *                    __restrict__ order,    /* lane i of the walking blocks <-> signature order[i] */
                 u32 const *              __restrict__ kscnt,    /* fd_keysplit_kernel's counters (FD_KC_*) */
                 u32 const *              __restrict__ hlist,    /* the hot keys' representatives */
                 uint4 const *            __restrict__ Axy,
                 uint4 *                  __restrict__ htab,     /* [hot key][2][8] entries: [1..8]([2^68](-A)), ([2^136](-A)) */
                 u32                                   hblk,     /* blocks [0,hblk) build them: one lane per (key, part) */
                 /* fixed-base keys (orderh = NULL: none): */
                 u32 const *              __restrict__ orderh,   /* the hot signatures as the split listed them */
                 u32 const *              __restrict__ flist,    /* (slot, representative) of the keys claimed in this batch */
                 uint4 *                  __restrict__ fbase,    /* [slot][32] [2^(8j)](-A) */
                 u32                                   fblk,     /* blocks [hblk,hblk+fblk) build them: lpk lanes per key */
                 unsigned char *          __restrict__ sstat,    /* [slot] the key's decode status */
                 uint4 *                  __restrict__ Rraw,
                 u32                                   lpk ) {   /* lanes per claimed key: 8 (j = 4t), or 32 (every j) */
  if( KS ) {
    if( blockIdx.x < hblk ) {
      /* dispatched first, so the chains of 68 and 136 doublings run beside the hash and not after it.  A key that
         does not decode or has small order builds nothing: its signatures' codes are final without a walk */
      u32 i = blockIdx.x * FD_WG + threadIdx.x;
      if( ( i >> 1 ) >= kscnt[FD_KC_HOTK] ) return;
      u32 rep = hlist[ i >> 1 ];
      if( astat[rep] & 7u ) return;
      htab_build( htab, i >> 1, i & 1u, Axy, rep );
      return;
    }
    if( blockIdx.x < hblk + fblk ) {
      /* likewise the fixed-base keys' chains of 32 t doublings, ahead of fd_ftab_kernel */
      u32 i = ( blockIdx.x - hblk ) * FD_WG + threadIdx.x;
      /* (of the keys that claimed a slot in this batch, by slot; the slot records the key's status,
         whether or not it decodes, for the batches that find it resident) */
      /* (lpk lanes per key, 8 for the tables j = 4t of group 0; 32 for all of them when a claim fills its
         slot at once, fdgpu_debug_opts_t.key_full = 2) */
      u32 k = i / lpk, q = i % lpk;
      if( k >= kscnt[FD_KC_BUILD] ) return;
      u32 slot = flist[ 2u*k ], rep = flist[ 2u*k + 1u ];
      if( !q ) sstat[slot] = astat[rep];
      if( astat[rep] & 7u ) return;
      fbase_build( fbase, slot, q * ( (u32)FD_FB_NT / lpk ), Axy, rep );
      return;
    }
    u32 col, j; int cls;
    if( !ks_pos( blockIdx.x - hblk - fblk, nsig, orderh ? kscnt[FD_KC_FB] : 0u, kscnt[FD_KC_HOT], col, j, cls ) ) return;
    u32 s = ks_sig( order, orderh, col, j, cls );
    if( cls==2 ) {
      hashf_one( payload, desc, map, s, nsig, semantics, astat[ arep[s] ], code_out, digA, digB, Rraw, khash, col );
      return;
    }
    if( orderh && cls==1 ) order[col] = s;                /* the hot segment of order[], for the kernels after this one */
    hashh_one<1>( payload, desc, map, s, nsig, semantics, 1, pstat, code_out, digA, digR, digB, slow, slow_cnt,
                  khash, force_slow, htop, arep, astat, col, cls==1 );
    return;
  }
  u32 s = blockIdx.x * FD_WG + threadIdx.x;
  if( s >= nsig ) return;
  hashh_one( payload, desc, map, s, nsig, semantics, 1, pstat, code_out, digA, digR, digB, slow, slow_cnt, khash,
             force_slow, htop, arep, astat );
}

/* Small batches (latency): the three independent parts of the prep in
   ONE launch -- blocks [0,sg) decode A, [sg,2sg) decode R, [2sg,3sg)
   check S and hash -- so a batch that cannot fill the GPU pays the
   longest of them instead of their sum.  Every block has one role, so
   no wave diverges. */
template<int FM, int HS>
FD_DEV void prep_role( unsigned char const * __restrict__ payload, fdgpu_txn_desc_t const * __restrict__ desc,
                       u32 const * __restrict__ map, u32 nsig, u32 role, u32 s, int semantics,
                       unsigned char * __restrict__ pstat, uint4 * __restrict__ Rxy, uint4 * __restrict__ Axy,
                       i8 * __restrict__ code_out, i8 * __restrict__ digA, short * __restrict__ digB,
                       uint4 * __restrict__ tab, uint4 const * __restrict__ khash, uint4 * __restrict__ tabR,
                       i8 * __restrict__ digR, u32 * __restrict__ slow, u32 * __restrict__ slow_cnt, u32 force_slow,
                       unsigned char * __restrict__ htop ) {
  if( role < 2u ) {
    decode_one<FM>( payload, desc, map, s, role, pstat + 2u*s + role, Rxy, Axy );
    /* tab != NULL: the A lane goes on to the -A table (for every A that
       decoded; fd_dsm2_kernel applies the result-code procedure); HS: the R
       lane to the -R table */
    if( tab && role==0u && ( pstat[2u*s] & 3u )==0u ) atab_build<FM>( tab, s, Axy );
    if( HS && role==1u && ( pstat[2u*s+1u] & 3u )==0u ) atab_build<FM>( tabR, s, Rxy );
  }
  else if( HS ) hashh_one( payload, desc, map, s, nsig, semantics, 0, pstat, code_out, digA, digR, digB, slow, slow_cnt,
                           khash, force_slow, htop );
  else hash_one( payload, desc, map, s, nsig, semantics, 0, pstat, code_out, digA, digB, Rxy, khash );
}

/* QS = 1 (half-size walk, batches of at most FD_QSHA_MAX signatures): the hash role on a quad of lanes per
   signature (hashh_one_q), blocks [2 sg, 6 sg) */
template<int FM, int HS, int QS = 0>
__global__ void __launch_bounds__( FD_WG )
fd_prep_kernel( unsigned char const *    __restrict__ payload,
                fdgpu_txn_desc_t const * __restrict__ desc,
                u32 const *              __restrict__ map,
                u32                                   nsig,
                u32                                   sg,
                int                                   semantics,
                unsigned char *          __restrict__ pstat,
                uint4 *                  __restrict__ Rxy,
                uint4 *                  __restrict__ Axy,
                i8 *                     __restrict__ code_out,
                i8 *                     __restrict__ digA,
                short *                  __restrict__ digB,
                uint4 *                  __restrict__ tab,
                uint4 const *            __restrict__ khash,
                uint4 *                  __restrict__ tabR,
                i8 *                     __restrict__ digR,
                u32 *                    __restrict__ slow,
                u32 *                    __restrict__ slow_cnt,
                u32                                   force_slow,
                unsigned char *          __restrict__ htop ) {
  u32 role, s;
  if( QS && blockIdx.x >= 2u*sg ) {              /* a quad per signature */
    role = 2u;
    s = ( blockIdx.x - 2u*sg ) * ( FD_WG / 4u ) + ( threadIdx.x >> 2 );
  } else {
    role = blockIdx.x / sg;
    s = ( blockIdx.x - role*sg ) * FD_WG + threadIdx.x;
  }
  if( s >= nsig ) return;                        /* (a quad's four lanes leave together) */
  if( QS && role == 2u ) {
    hashh_one_q( payload, desc, map, s, nsig, code_out, digA, digR, digB, slow, slow_cnt, khash, force_slow, htop,
                 threadIdx.x & 3u, threadIdx.x & 60u );
    return;
  }
  prep_role<FM,HS>( payload, desc, map, nsig, role, s, semantics, pstat, Rxy, Axy, code_out, digA, digB,
                    tab, khash, tabR, digR, slow, slow_cnt, force_slow, htop );
}

/* Stage 3 -- table [0..8](-A) in cached form (fd_ed25519_point_neg + the
   odd-multiple table of fd_curve25519.c:118-131; here all multiples, for a
   signed fixed window). */
__global__ void __launch_bounds__( FD_WG, 3 )
fd_table_kernel( u32 nsig, int semantics, unsigned char const * __restrict__ pstat, i8 * __restrict__ code,
                 uint4 const * __restrict__ Axy, uint4 * __restrict__ tab ) {
  u32 s = blockIdx.x * FD_WG + threadIdx.x;
  if( s >= nsig ) return;
  if( pstat ) {                                  /* small batches: fd_prep_kernel left S's check only */
    int c = result_code( code[s], pstat[2*s], pstat[2*s+1], semantics, 0 );
    code[s] = (i8)c;
    if( c != FD_ED25519_SUCCESS ) return;
  } else if( code[s] != FD_ED25519_SUCCESS ) return;
  atab_build( tab, s, Axy );
}

/* [k](-A) + [S]B for signature s (full-length signed fixed windows; body of
   fd_dsm_kernel and of fd_dsm_slow_kernel).  defer: store P for the R-check
   kernels; else compare with the decoded R and write the code. */
template<int FM>
FD_DEV void dsm_one( u32 s, size_t n, uint4 const * __restrict__ tab, uint4 const * __restrict__ Rxy,
                     i8 const * __restrict__ digA, short const * __restrict__ digB, uint4 const * btab,
                     i8 * __restrict__ code, u32 * __restrict__ Pbuf, int defer, u32 sa,      /* sa: whose -A table */
                     u32 col ) {                                       /* col: the signature's digit column (s, or its
                                                                          place in the hot / cold order) */
  ge_p3 P; ge_p3_identity( P );
  ge_p2 P2;
  atab_raw raw;
  int da = digA[ (size_t)63*n + col ];

  uint4 braw[6]; int db = 0;
#pragma unroll 1
  for( int w=63; w>=0; w-- ) {
    atab_fetch( raw, tab, sa, da < 0 ? -da : da );   /* issued before the window's doublings: in flight during them */
    if( !(w & 3) ) {                                 /* base-point entry, also in flight */
      db = digB[ (size_t)(w>>2)*n + col ];
      uint4 const * bp = btab + (size_t)( db < 0 ? -db : db )*6;
#pragma unroll
      for( int i=0; i<6; i++ ) braw[i] = bp[i];
    }
    ge_p1p1 t;
    if( w != 63 ) {
#pragma unroll 1
      for( int r=0; r<3; r++ ) { ge_dbl<FM>( t, P2 ); ge_p1p1_to_p2<FM>( P2, t ); }
      ge_dbl<FM>( t, P2 ); ge_p1p1_to_p3<FM>( P, t );
    }
    {
      ge_cached q; atab_unpack( q, raw ); ge_cached_cneg( q, da < 0 );
      ge_add_cached<FM>( t, P, q );
    }
    if( !(w & 3) ) {
      ge_p1p1_to_p3<FM>( P, t );
      ge_precomp bq;
      fe_from_quads( bq.ypx,  braw[0], braw[1] );
      fe_from_quads( bq.ymx,  braw[2], braw[3] );
      fe_from_quads( bq.xy2d, braw[4], braw[5] );
      ge_precomp_cneg( bq, db < 0 );
      ge_add_precomp<FM>( t, P, bq );
    }
    ge_p1p1_to_p2<FM>( P2, t );
    if( w > 0 ) da = digA[ (size_t)(w-1)*n + col ];
  }

  if( defer ) {
    /* P for the R-check kernels, planar limbs (coalesced) */
    fe_store_planar( Pbuf + s, n, P2.X );
    fe_store_planar( Pbuf + 10*n + s, n, P2.Y );
    fe_store_planar( Pbuf + 20*n + s, n, P2.Z );
    return;
  }
  /* R decoded up front (small batches): fd_ed25519_point_eq_z1,
     X == x_R Z and Y == y_R Z */
  uint4 const * rp = Rxy + (size_t)s*4;
  fe x, y, u;
  fe_from_quads( x, rp[0], rp[1] );
  fe_from_quads( y, rp[2], rp[3] );
  fe_mul<FM>( u, x, P2.Z ); int okx = fe_eq( u, P2.X );
  fe_mul<FM>( u, y, P2.Z ); int oky = fe_eq( u, P2.Y );
  code[s] = (okx & oky) ? FD_ED25519_SUCCESS : FD_ED25519_ERR_MSG;
}

/* (no minimum waves per SIMD asked of the compiler: the register count decides, 162 VGPRs -> 3 waves) */
template<int FM>
__global__ void __launch_bounds__( FD_WG )
fd_dsm_kernel( u32                      nsig,
               uint4 const * __restrict__ tab,
               uint4 const * __restrict__ Rxy,
               i8 const *    __restrict__ digA,
               short const * __restrict__ digB,
               uint4 const * __restrict__ btab,
               i8 *          __restrict__ code,
               u32 *         __restrict__ Pbuf,
               int                        defer ) {
  u32 s = blockIdx.x * FD_WG + threadIdx.x;
  if( s >= nsig ) return;
  if( code[s] != FD_ED25519_SUCCESS ) return;
  dsm_one<FM>( s, nsig, tab, Rxy, digA, digB, btab, code, Pbuf, defer, s, s );
}

/* Half-size path: the signatures on the slow list (no short (c0, c1)) take
   the full 253-bit walk over k's and S's digits, R compared at its end,
   compacted into whole waves.  fd_dsmh_kernel's first blocks take the head
   of the list; this kernel the rest (normally nothing: ~0.2 % of
   signatures, more only for inputs ground to defeat the reduction). */
template<int FM>
__global__ void __launch_bounds__( FD_WG )
fd_dsm_slow_kernel( u32 nsig, uint4 const * __restrict__ tab, uint4 const * __restrict__ Rxy,
                    i8 const * __restrict__ digA, short const * __restrict__ digB, uint4 const * __restrict__ btab,
                    i8 * __restrict__ code, u32 const * __restrict__ slow, u32 const * __restrict__ slow_cnt,
                    u32 first, u32 const * __restrict__ arep, u32 const * __restrict__ order ) {
  u32 i = first + blockIdx.x * FD_WG + threadIdx.x;
  /* order (hot / cold partition, fd_keysplit_kernel): the list names digit columns, order[] the signature */
  if( i < *slow_cnt ) {
    u32 col = slow[i], s = order ? order[col] : col;
    dsm_one<FM>( s, nsig, tab, Rxy, digA, digB, btab, code, (u32 *)0, 0, arep ? arep[s] : s, col );
  }
}

/* Latency half-size path: the slow list after the walks, the result-code
   procedure first (fd_prep_kernel ran it beside the decodes: S only).  The 8/4/2-lane walk kernels run it
   at their end (one kernel less on a batch's chain: a launch costs the chain ~5-10 us, profiles/r05/tc);
   fd_dsm_slowl_kernel after the one-lane walk.  Thread i of the grid takes entries i, i + grid, ... */
template<int FM>
FD_DEV void slowl_tail( u32 nsig, uint4 const * __restrict__ tab, uint4 const * __restrict__ Rxy,
                        i8 const * __restrict__ digA, short const * __restrict__ digB, uint4 const * __restrict__ btab,
                        i8 * __restrict__ code, u32 const * __restrict__ slow, u32 const * __restrict__ slow_cnt,
                        int semantics, unsigned char const * __restrict__ pstat ) {
  u32 n = *slow_cnt;
  for( u32 i = blockIdx.x * FD_WG + threadIdx.x; i < n; i += gridDim.x * FD_WG ) {
    u32 s = slow[i];
    if( code[s] != FD_PEND_SLOW ) continue;
    int c = result_code( FD_ED25519_SUCCESS, pstat[2*s], pstat[2*s+1], semantics, 0 );
    if( c != FD_ED25519_SUCCESS ) { code[s] = (i8)c; continue; }
    dsm_one<FM>( s, nsig, tab, Rxy, digA, digB, btab, code, (u32 *)0, 0, s, s );
  }
}

template<int FM>
__global__ void __launch_bounds__( FD_WG )
fd_dsm_slowl_kernel( u32 nsig, uint4 const * __restrict__ tab, uint4 const * __restrict__ Rxy,
                     i8 const * __restrict__ digA, short const * __restrict__ digB, uint4 const * __restrict__ btab,
                     i8 * __restrict__ code, u32 const * __restrict__ slow, u32 const * __restrict__ slow_cnt,
                     int semantics, unsigned char const * __restrict__ pstat ) {
  slowl_tail<FM>( nsig, tab, Rxy, digA, digB, btab, code, slow, slow_cnt, semantics, pstat );
}

/* Half-size DSM: Q = [s']B + [c0](-A) + [c1](-R) by a joint signed
   fixed-window walk over (normally) 33 windows of 4 bits -- 128 doublings,
   33 -A adds and 33 -R adds (both tables gathered from HBM, the -A entry
   across the window's doublings), and the 16 radix-2^16 digits of s' as one
   base-point add per even window from [0..32768]B (digits 0-7) and
   [0..32768](2^120 B) (digits 8-15).
   Q == O (X == 0, Y == Z)  <=>  R == [S]B - [k]A  (fd_gpu_lattice.h). */
/* FD_DSMH_MINW: waves per SIMD asked of the compiler (3: <= 168 VGPRs) */
#define FD_DSMH_MINW 3
/* The walk of a hot signature (a key the batch repeats): c0 in three parts of W = 17 windows,
     Q = [s']B + [c0_0](-A) + [c0_1]([2^68](-A)) + [c0_2]([2^136](-A)) + [c1](-R),
   over 17 windows (up to FD_KS_NW when a lane's pair needs them) = 64 doublings.  Per window: 4 doublings, the
   three -A-part adds (part 0 from the key's -A table at sa, parts 1 and 2 from its high tables at 2 hi, 2 hi + 1
   of htab), the -R add, and s' digit j from btab / btabh at window hs_hot_bwin( j ).  Each gather is issued one
   add ahead, so two raw entries are live at a time, as in the cold walk. */
template<int FM>
FD_DEV int dsmh_hot( u32 s, u32 col, size_t n, int wtop, u32 sa, u32 hi,
                     uint4 const * __restrict__ tabA, uint4 const * __restrict__ tabR, uint4 const * __restrict__ htab,
                     i8 const * __restrict__ digA, i8 const * __restrict__ digR, short const * __restrict__ digB,
                     uint4 const * __restrict__ btab, uint4 const * __restrict__ btabh ) {
  ge_p3 P; ge_p3_identity( P );
  ge_p2 P2;
  atab_raw ra, rb;
  i8 const * dA = digA + col;
  /* parts 0 and 1 end at window W - 1: above it only part 2 and c1 have digits */
  int d2 = dA[ (size_t)( 2*FD_KS_W + wtop )*n ], dr = digR[ (size_t)wtop*n + col ];
  int d0 = wtop < FD_KS_W ? (int)dA[ (size_t)wtop*n ] : 0, d1 = wtop < FD_KS_W ? (int)dA[ (size_t)( FD_KS_W + wtop )*n ] : 0;
#pragma unroll 1
  for( int w=wtop; w>=0; w-- ) {
    atab_fetch( ra, htab, 2u*hi + 1u, d2 < 0 ? -d2 : d2 );   /* in flight during the doublings */
    ge_p1p1 t;
    if( w != wtop ) {
#pragma unroll 1
      for( int r=0; r<3; r++ ) { ge_dbl<FM>( t, P2 ); ge_p1p1_to_p2<FM>( P2, t ); }
      ge_dbl<FM>( t, P2 ); ge_p1p1_to_p3<FM>( P, t );
    }
    atab_fetch( rb, htab, 2u*hi, d1 < 0 ? -d1 : d1 );
    { ge_cached q; atab_unpack( q, ra ); ge_cached_cneg( q, d2 < 0 ); ge_add_cached<FM>( t, P, q ); ge_p1p1_to_p3<FM>( P, t ); }
    atab_fetch( ra, tabA, sa, d0 < 0 ? -d0 : d0 );
    { ge_cached q; atab_unpack( q, rb ); ge_cached_cneg( q, d1 < 0 ); ge_add_cached<FM>( t, P, q ); ge_p1p1_to_p3<FM>( P, t ); }
    atab_fetch( rb, tabR, s, dr < 0 ? -dr : dr );
    { ge_cached q; atab_unpack( q, ra ); ge_cached_cneg( q, d0 < 0 ); ge_add_cached<FM>( t, P, q ); ge_p1p1_to_p3<FM>( P, t ); }
    /* s' digit: class w & 3 picks the table, (w >> 2) the digit within its run */
    int cl = w & 3;
    int bw = w <= ( cl==0 ? 16 : cl==2 ? 14 : cl==1 ? 13 : 11 );
    int db = bw ? digB[ (size_t)( ( cl==0 ? 0 : cl==2 ? 5 : cl==1 ? 9 : 13 ) + ( w >> 2 ) )*n + col ] : 0;
    { ge_cached q; atab_unpack( q, rb ); ge_cached_cneg( q, dr < 0 ); ge_add_cached<FM>( t, P, q ); }
    if( bw ) {
      uint4 braw[6];
      uint4 const * bt = cl==0 ? btab : btabh + (size_t)( cl==2 ? 0 : cl==1 ? 1 : 2 ) * ( (size_t)FD_BTAB_ENTRIES * 6 );
      uint4 const * bp = bt + (size_t)( db < 0 ? -db : db )*6;
#pragma unroll
      for( int i=0; i<6; i++ ) braw[i] = bp[i];
      ge_precomp bq;
      ge_p1p1_to_p3<FM>( P, t );
      fe_from_quads( bq.ypx,  braw[0], braw[1] );
      fe_from_quads( bq.ymx,  braw[2], braw[3] );
      fe_from_quads( bq.xy2d, braw[4], braw[5] );
      ge_precomp_cneg( bq, db < 0 );
      ge_add_precomp<FM>( t, P, bq );
    }
    ge_p1p1_to_p2<FM>( P2, t );
    if( w > 0 ) {
      int lo = w - 1 < FD_KS_W;
      d2 = dA[ (size_t)( 2*FD_KS_W + w - 1 )*n ]; dr = digR[ (size_t)( w - 1 )*n + col ];
      d0 = lo ? (int)dA[ (size_t)( w - 1 )*n ] : 0; d1 = lo ? (int)dA[ (size_t)( FD_KS_W + w - 1 )*n ] : 0;
    }
  }
  return fe_is_zero( P2.X ) & fe_eq( P2.Y, P2.Z );
}

/* The walk of a fixed-base signature: P = [S]B + [k](-A) from the key's tables (ftab, key fi) and
   the base point's (btabf[t] = [0..32768]([2^(32t)]B)), in four steps at bit offsets 24, 16, 8 and 0 of each
   32-bit span with 8 doublings between steps.  The step at offset 8r adds digit a_(4t+r) of k from table t for
   t = 0..7, and the steps at offsets 16 and 0 also digit b_(2t+1), b_(2t) of S from btabf[t]: 32 + 16 affine
   adds, 24 doublings.  Each 96-byte entry is gathered one add ahead.  P goes to Pbuf's column col for the R-check
   kernels, as dsm_one( defer = 1 ) leaves it. */
FD_DEV void ptab_fetch( uint4 r[ 6 ], uint4 const * p ) {
#pragma unroll
  for( int i=0; i<6; i++ ) r[i] = p[i];
}
template<int FM>
FD_DEV void dsmf_one( u32 col, size_t n, u32 fi, uint4 const * __restrict__ ftab, uint4 const * __restrict__ btabf,
                      i8 const * __restrict__ digA, short const * __restrict__ digB, u32 * __restrict__ Pbuf ) {
  ge_p3 P; ge_p3_identity( P );
  i8 const * dA = digA + col; short const * dB = digB + col;
  uint4 ra[ 6 ], rb[ 6 ];
#pragma unroll 1
  for( int r=3; r>=0; r-- ) {
    int na = fd_fb_old_adds( r );                      /* adds of this step: 8 from the key's tables, then 8 from B's */
    int d = dA[ (size_t)fd_fb_old_digit( r, 0 )*n ];
    ptab_fetch( ra, d ? ftab + ftab_at( fi, (u32)fd_fb_old_table( 0 ), (u32)fd_fb_entry( d ) ) : (uint4 const *)fd_ptab_ident_w );
#pragma unroll 1
    for( int i=0; i<na; i++ ) {
      int dn = 0;
      if( i + 1 < na ) {                               /* the next add's entry, in flight during this one */
        int i1 = i + 1;
        if( !fd_fb_old_is_base( i1 ) ) {               /* (the slot's tables 4t and the base point's 2t: fd_gpu_lattice.h) */
          dn = dA[ (size_t)fd_fb_old_digit( r, i1 )*n ];
          ptab_fetch( rb, dn ? ftab + ftab_at( fi, (u32)fd_fb_old_table( i1 ), (u32)fd_fb_entry( dn ) ) : (uint4 const *)fd_ptab_ident_w );
        } else {
          dn = dB[ (size_t)fd_fb_old_digit( r, i1 )*n ];
          ptab_fetch( rb, btabf + ( (size_t)fd_fb_old_table( i1 ) * FD_BTAB_ENTRIES + (size_t)fd_fb_entry( dn ) ) * 6 );
        }
      }
      ge_precomp q;
      fe_from_quads( q.ypx,  ra[0], ra[1] );
      fe_from_quads( q.ymx,  ra[2], ra[3] );
      fe_from_quads( q.xy2d, ra[4], ra[5] );
      ge_precomp_cneg( q, d < 0 );
      ge_p1p1 t;
      ge_add_precomp<FM>( t, P, q ); ge_p1p1_to_p3<FM>( P, t );
#pragma unroll
      for( int v=0; v<6; v++ ) ra[v] = rb[v];
      d = dn;
    }
    if( r ) {
      ge_p2 P2; P2.X = P.X; P2.Y = P.Y; P2.Z = P.Z;
      ge_p1p1 t;
#pragma unroll 1
      for( int b=0; b<7; b++ ) { ge_dbl<FM>( t, P2 ); ge_p1p1_to_p2<FM>( P2, t ); }
      ge_dbl<FM>( t, P2 ); ge_p1p1_to_p3<FM>( P, t );
    }
  }
  fe_store_planar( Pbuf + col, n, P.X );
  fe_store_planar( Pbuf + 10*n + col, n, P.Y );
  fe_store_planar( Pbuf + 20*n + col, n, P.Z );
}

/* The walk of a fixed-base signature whose key's slot is full: every byte of k has a table of its own
   and every 16-bit digit of S one of the base point's, so P = [S]B + [k](-A) is the sum of 32 + 16 entries with no
   doubling at all.  Addition i reads what fd_fb_full_digit / fd_fb_full_table say (two of the key's, then one of
   the base point's).  Each 96-byte entry is gathered one addition ahead; the loop takes two additions a turn, so
   the two raw entries never move.  (A third raw entry, gathered two ahead, costs the third wave: 120 B of
   scratch.)  P is stored as dsmf_one stores it. */
FD_DEV void full_fetch( uint4 r[ 6 ], int & d, int i, size_t n, u32 fi, uint4 const * __restrict__ ftab,
                        uint4 const * __restrict__ btabf, i8 const * __restrict__ dA, short const * __restrict__ dB ) {
  if( !fd_fb_full_is_base( i ) ) {
    d = dA[ (size_t)fd_fb_full_digit( i )*n ];
    ptab_fetch( r, d ? ftab + ftab_at( fi, (u32)fd_fb_full_table( i ), (u32)fd_fb_entry( d ) ) : (uint4 const *)fd_ptab_ident_w );
  } else {
    d = dB[ (size_t)fd_fb_full_digit( i )*n ];
    ptab_fetch( r, btabf + ( (size_t)fd_fb_full_table( i ) * FD_BTAB_ENTRIES + (size_t)fd_fb_entry( d ) ) * 6 );
  }
}
template<int FM>
FD_DEV void full_add( ge_p3 & P, uint4 const r[ 6 ], int d ) {
  ge_precomp q;
  fe_from_quads( q.ypx,  r[0], r[1] );
  fe_from_quads( q.ymx,  r[2], r[3] );
  fe_from_quads( q.xy2d, r[4], r[5] );
  ge_precomp_cneg( q, d < 0 );
  ge_p1p1 t;
  ge_add_precomp<FM>( t, P, q ); ge_p1p1_to_p3<FM>( P, t );
}
template<int FM>
FD_DEV void dsmf_full( u32 col, size_t n, u32 fi, uint4 const * __restrict__ ftab, uint4 const * __restrict__ btabf,
                       i8 const * __restrict__ digA, short const * __restrict__ digB, u32 * __restrict__ Pbuf ) {
  ge_p3 P; ge_p3_identity( P );
  i8 const * dA = digA + col; short const * dB = digB + col;
  uint4 ra[ 6 ], rb[ 6 ];
  int da, db;
  full_fetch( ra, da, 0, n, fi, ftab, btabf, dA, dB );
#pragma unroll 1
  for( int i=0; i<FD_FB_FULL_ADDS; i+=2 ) {
    full_fetch( rb, db, i + 1, n, fi, ftab, btabf, dA, dB );
    full_add<FM>( P, ra, da );
    if( i + 2 < FD_FB_FULL_ADDS ) full_fetch( ra, da, i + 2, n, fi, ftab, btabf, dA, dB );
    full_add<FM>( P, rb, db );
  }
  fe_store_planar( Pbuf + col, n, P.X );
  fe_store_planar( Pbuf + 10*n + col, n, P.Y );
  fe_store_planar( Pbuf + 20*n + col, n, P.Z );
}

/* The walk of a fixed-base signature whose key's slot has wide tables: every 32-bit span of k is three
   digits of 11, 11 and 10 bits with a table each, so P is the sum of 24 + 16 entries.  Addition i reads what
   fd_fb_wide_* say: per span the key's three tables, then the base point's two.  The three digits come from the four
   bytes of the span that the hash role stored (fd_fb_wide_split); they are loaded again for each of the three
   additions rather than kept, which costs loads that hit and no register.  Zero digits read the identity entry at
   the head of wtab[], so every gather of the key's is wtab + an offset.  Gathered one addition ahead, two additions
   a turn, P stored as dsmf_full does. */
FD_DEV void wide_fetch( uint4 r[ 6 ], int & d, int i, size_t n, u32 fi, uint4 const * __restrict__ wtab,
                        uint4 const * __restrict__ btabf, i8 const * __restrict__ dA, short const * __restrict__ dB ) {
  if( !fd_fb_wide_is_base( i ) ) {
    int t = fd_fb_wide_span( i ), q = fd_fb_wide_digit( i );
    i8 const * p = dA + (size_t)( 4*t )*n;
    d = fd_fb_wide_split( p[0], p[n], p[2*n], p[3*n], q );
    ptab_fetch( r, wtab + ( d ? wtab_at( fi, (u32)t, (u32)q, (u32)fd_fb_entry( d ) ) : (size_t)0 ) );
  } else {
    d = dB[ (size_t)fd_fb_wide_digit( i )*n ];
    ptab_fetch( r, btabf + ( (size_t)fd_fb_wide_table( i ) * FD_BTAB_ENTRIES + (size_t)fd_fb_entry( d ) ) * 6 );
  }
}
template<int FM>
FD_DEV void dsmf_wide( u32 col, size_t n, u32 fi, uint4 const * __restrict__ wtab, uint4 const * __restrict__ btabf,
                       i8 const * __restrict__ digA, short const * __restrict__ digB, u32 * __restrict__ Pbuf ) {
  ge_p3 P; ge_p3_identity( P );
  i8 const * dA = digA + col; short const * dB = digB + col;
  uint4 ra[ 6 ], rb[ 6 ];
  int da, db;
  wide_fetch( ra, da, 0, n, fi, wtab, btabf, dA, dB );
#pragma unroll 1
  for( int i=0; i<FD_FB_WIDE_ADDS; i+=2 ) {
    wide_fetch( rb, db, i + 1, n, fi, wtab, btabf, dA, dB );
    full_add<FM>( P, ra, da );
    if( i + 2 < FD_FB_WIDE_ADDS ) wide_fetch( ra, da, i + 2, n, fi, wtab, btabf, dA, dB );
    full_add<FM>( P, rb, db );
  }
  fe_store_planar( Pbuf + col, n, P.X );
  fe_store_planar( Pbuf + 10*n + col, n, P.Y );
  fe_store_planar( Pbuf + 20*n + col, n, P.Z );
}

template<int FM, int KS = 0>
__global__ void __launch_bounds__( FD_WG, FM ? FD_DSMH_MINW : 1 )
fd_dsmh_kernel( u32                      nsig,
                uint4 const * __restrict__ tabA,
                uint4 const * __restrict__ tabR,
                i8 const *    __restrict__ digA,
                i8 const *    __restrict__ digR,
                short const * __restrict__ digB,
                uint4 const * __restrict__ btab,
                uint4 const * __restrict__ btab2,
                i8 *          __restrict__ code,
                uint4 const * __restrict__ Rxy,
                u32 const *   __restrict__ slow,
                u32 const *   __restrict__ slow_cnt,
                u32                        nslowblk,
                unsigned char const * __restrict__ pstat,
                unsigned char const * __restrict__ htop,
                int                        rc,
                int                        semantics,
                u32 const *   __restrict__ arep,         /* keys de-duplicated: -A's table is at arep[s], else NULL */
                /* KS (hot / cold partition, fd_keysplit_kernel; the grid is nslowblk + sg + 1 blocks): */
                u32 const *   __restrict__ order,        /* lane i of the walking blocks <-> signature order[i] */
                u32 const *   __restrict__ kscnt,        /* [1] hot signatures */
                u32 const *   __restrict__ hidx,         /* a hot representative's dense index */
                uint4 const * __restrict__ htab,         /* the high tables (htab_build) */
                uint4 const * __restrict__ btabh,        /* [0..32768](2^e B), e = 72, 140, 196 */
                /* fixed-base keys (fidx = NULL: none; the grid is then nslowblk + sg + 2 blocks): */
                u32 const *   __restrict__ fidx,         /* a fixed-base representative's dense index */
                uint4 const * __restrict__ ftab,         /* the keys' tables (fd_ftab_kernel) */
                uint4 const * __restrict__ btabf,        /* [16][0..32768]([2^(16u)]B) */
                u32 *         __restrict__ Pbuf,         /* P of a fixed-base signature, at its place */
                u32 const *   __restrict__ full,         /* [slot] 0: tables j = 0 (mod 4) only, else all 32 */
                u32 *         __restrict__ ffcnt,        /* the signatures that walked without doublings (FD_KC_FFS) */
                uint4 const * __restrict__ wtab,         /* the wide tables of the slots below wcap */
                u32                        wcap ) {
  size_t n = nsig;
  if( blockIdx.x < nslowblk ) {
    /* the first blocks take the head of the slow list (full 253-bit walk,
       about twice a half-size walk): dispatched first, they run beside the
       half-size waves instead of after them; fd_dsm_slow_kernel takes the rest */
    u32 i = blockIdx.x * FD_WG + threadIdx.x;
    if( i < *slow_cnt ) {
      u32 cs = slow[i], ss = KS ? order[cs] : cs;
      dsm_one<FM>( ss, n, tabA, Rxy, digA, digB, btab, code, (u32 *)0, 0, arep ? arep[ss] : ss, cs );
    }
    return;
  }
  /* col: the lane's digit column -- the signature itself, or (KS) its place in the hot / cold order */
  u32 s, col; int in, hot = 0;
  if( KS ) {
    u32 j; int cls;
    in = ks_pos( blockIdx.x - nslowblk, nsig, fidx ? kscnt[FD_KC_FB] : 0u, kscnt[FD_KC_HOT], col, j, cls );
    s = in ? order[col] : 0u;
    if( cls==2 ) {                                      /* (block-uniform) a fixed-base block: pending = SUCCESS so far */
      /* before any lane leaves, the wave votes.  When every lane that walks has a full slot, the wave
         walks without doublings; one lane that does not, and it walks as before, from the tables j = 0 (mod 4)
         that every slot has.  The wave's count of such signatures: one no-return add by its first walking lane. */
      int walk = in && code[s] == FD_ED25519_SUCCESS;
      u32 fi = walk ? fidx[ arep[s] ] : 0u;
      unsigned long long wm = __ballot( walk );
      int allfull = __all( walk ? full[fi] != 0u : 1 );
      /* one level more.  When every one of them is also below wcap, the wave walks 40 additions from the
         wide tables; a wave that mixes the two kinds of full slot walks 48 from the byte tables, which both have.
         The word FD_KC_FWS counts the former beside ffcnt[0] (FD_KC_FFS), which counts both */
      int allwide = allfull && __all( walk ? fi < wcap : 1 );
      if( !walk ) return;
      if( allfull ) {
        if( (int)( threadIdx.x & 63u ) == __ffsll( (long long)wm ) - 1 ) {
          atomicAdd( ffcnt, (u32)__popcll( wm ) );
          if( allwide ) atomicAdd( ffcnt + ( FD_KC_FWS - FD_KC_FFS ), (u32)__popcll( wm ) );
        }
        if( allwide ) dsmf_wide<FM>( col, n, fi, wtab, btabf, (i8 const *)digA, digB, Pbuf );
        else dsmf_full<FM>( col, n, fi, ftab, btabf, (i8 const *)digA, digB, Pbuf );
      }
      else dsmf_one<FM>( col, n, fi, ftab, btabf, (i8 const *)digA, digB, Pbuf );
      return;
    }
    hot = cls==1;
  }
  else { s = col = ( blockIdx.x - nslowblk ) * FD_WG + threadIdx.x; in = s < nsig; }
  /* a slow-list signature's code may already be final (SUCCESS) when this
     block starts: the flag, not the code, keeps it out */
  /* rc (latency path, after fd_prep_kernel): the result-code procedure
     here; slow signatures (FD_PEND_SLOW) are left to fd_dsm_slowl_kernel */
  int c = in ? (int)code[s] : FD_ED25519_ERR_SIG;
  if( rc && in ) c = result_code( c, pstat[2*s], pstat[2*s+1], semantics, 0 );
  int pend = c == FD_ED25519_SUCCESS && !( pstat[2*s] & FD_PSTAT_SLOW );
  /* the walk starts at the wave's highest nonzero window of c0, c1 and s' (31-32 unless a lane's
     scalar exceeds 2^131; window 30 or above while s' >= 2^240): every lane of the wave is still here */
  int wtop = hs_wave_top( pend, htop, col );
  if( !pend ) { if( rc && in && c != FD_PEND_SLOW ) code[s] = (i8)c; return; }
  u32 sa = arep ? arep[s] : s;
  if( KS && hot ) {                                     /* (block-uniform) */
    int ok = dsmh_hot<FM>( s, col, n, wtop, sa, hidx[sa], tabA, tabR, htab, digA, digR, digB, btab, btabh );
    code[s] = ok ? FD_ED25519_SUCCESS : FD_ED25519_ERR_MSG;
    return;
  }
  ge_p3 P; ge_p3_identity( P );
  ge_p2 P2;
  atab_raw ra, rr;
  int da = digA[ (size_t)wtop*n + col ], dr = digR[ (size_t)wtop*n + col ];
#pragma unroll 1
  for( int w=wtop; w>=0; w-- ) {
    atab_fetch( ra, tabA, sa, da < 0 ? -da : da );    /* in flight during the doublings */
    ge_p1p1 t;
    if( w != wtop ) {
#pragma unroll 1
      for( int r=0; r<3; r++ ) { ge_dbl<FM>( t, P2 ); ge_p1p1_to_p2<FM>( P2, t ); }
      ge_dbl<FM>( t, P2 ); ge_p1p1_to_p3<FM>( P, t );
    }
    /* the -R entry is issued after the doublings, in flight during the -A
       add (prefetching it across the doublings as well, or issuing it after
       the -A add: the same time, A/B 7.13-7.21 ms) */
    atab_fetch( rr, tabR, s, dr < 0 ? -dr : dr );
    {
      ge_cached q; atab_unpack( q, ra ); ge_cached_cneg( q, da < 0 );
      ge_add_cached<FM>( t, P, q ); ge_p1p1_to_p3<FM>( P, t );
    }
    /* base-point digit j (bits 16j..16j+15 of s') at window 4j from [0..32768]B,
       digit j+8 (bits 16j+128..) at window 4j+2 from [0..32768](2^120 B):
       one base-point add per even window */
    int bw = !(w & 1) && w < 32;
    int db = bw ? digB[ (size_t)( (w>>2) + ( (w & 2) ? 8 : 0 ) )*n + col ] : 0;
    {
      ge_cached q; atab_unpack( q, rr ); ge_cached_cneg( q, dr < 0 );
      ge_add_cached<FM>( t, P, q );
    }
    if( bw ) {
      uint4 braw[6];                                 /* in flight during the P3 conversion (across the
                                                        -R add it cost the 3rd wave) */
      uint4 const * bp = ( (w & 2) ? btab2 : btab ) + (size_t)( db < 0 ? -db : db )*6;
#pragma unroll
      for( int i=0; i<6; i++ ) braw[i] = bp[i];
      ge_precomp bq;
      ge_p1p1_to_p3<FM>( P, t );
      fe_from_quads( bq.ypx,  braw[0], braw[1] );
      fe_from_quads( bq.ymx,  braw[2], braw[3] );
      fe_from_quads( bq.xy2d, braw[4], braw[5] );
      ge_precomp_cneg( bq, db < 0 );
      ge_add_precomp<FM>( t, P, bq );
    }
    ge_p1p1_to_p2<FM>( P2, t );
    if( w > 0 ) { da = digA[ (size_t)(w-1)*n + col ]; dr = digR[ (size_t)(w-1)*n + col ]; }
  }
  /* Q == O: X == 0 and Y == Z (Z != 0: complete formulas) */
  int ok = fe_is_zero( P2.X ) & fe_eq( P2.Y, P2.Z );
  code[s] = ok ? FD_ED25519_SUCCESS : FD_ED25519_ERR_MSG;
}

/* ---- latency path: two lanes per signature ------------------------------
   A batch too small to fill the GPU finishes when one wave has issued its
   whole DSM, so the latency path halves each lane's share of the field
   work: lanes 2s and 2s+1 (h = 0, 1) of a wave share signature s and
   exchange field elements with one DPP quad_perm[1,0,3,2] move per limb.
   Every group-law step is split into two multiplications per lane:
     doubling    lane 0 squares X and X+Y, lane 1 Y and Z; both lanes form
                 E, F, G, H (eprint 2008/522 §4.4);
     addition    lane 0 A = (Y+X)(Y2+X2) and C = T 2dT2, lane 1
                 B = (Y-X)(Y2-X2) and D = Z Z2 (§4.2); a base-point
                 entry (Z2 = 1) is the same step with Z2 = 1;
     M-step      completed -> extended: lane 0 X3 = EF and T3 = EH, lane 1
                 Y3 = GH and Z3 = GF.
   The M-step output (lane 0 X3, T3; lane 1 Y3, Z3) is exactly what both
   the next doubling and an addition take in, so between steps each lane
   receives one element of its partner.  Each lane gathers only the two
   coordinates of a table entry it multiplies by.  Per lane: 2 S + 2 M
   and ~100 moves / selects per doubling instead of 4 S + 3 M -- about
   0.73x the instruction stream of fd_dsm_kernel, at 1.35x its total
   work, so it is only used when the batch leaves SIMDs idle. */
/* Lane exchanges as DPP quad_perm moves in inline asm,
   one s_nop 1 ahead of them for the VALU-write -> DPP-read hazard.  (The
   compiler's own lowering of __builtin_amdgcn_update_dpp gave wrong
   results here on gfx950 -- measured: every valid signature rejected --
   while these moves and a ds_swizzle __shfl_xor agree with the oracle.) */
#define FD_DPP_MOV( d, a, PERM ) "v_mov_b32_dpp %" #d ", %" #a " " PERM " row_mask:0xf bank_mask:0xf\n\t"
/* r = a as seen through one quad_perm (10 moves, one asm block) */
#define FD_DEF_FE_DPP( name, PERM )                                                        \
FD_DEV void name( fe & r, fe const & a ) {                                                 \
  asm volatile( "s_nop 1\n\t"                                                              \
                FD_DPP_MOV( 0, 10, PERM ) FD_DPP_MOV( 1, 11, PERM ) FD_DPP_MOV( 2, 12, PERM ) \
                FD_DPP_MOV( 3, 13, PERM ) FD_DPP_MOV( 4, 14, PERM ) FD_DPP_MOV( 5, 15, PERM ) \
                FD_DPP_MOV( 6, 16, PERM ) FD_DPP_MOV( 7, 17, PERM ) FD_DPP_MOV( 8, 18, PERM ) \
                FD_DPP_MOV( 9, 19, PERM )                                                  \
                : "=&v"( r.v[0] ), "=&v"( r.v[1] ), "=&v"( r.v[2] ), "=&v"( r.v[3] ), "=&v"( r.v[4] ), \
                  "=&v"( r.v[5] ), "=&v"( r.v[6] ), "=&v"( r.v[7] ), "=&v"( r.v[8] ), "=&v"( r.v[9] ) \
                : "v"( a.v[0] ), "v"( a.v[1] ), "v"( a.v[2] ), "v"( a.v[3] ), "v"( a.v[4] ),  \
                  "v"( a.v[5] ), "v"( a.v[6] ), "v"( a.v[7] ), "v"( a.v[8] ), "v"( a.v[9] ) ); \
}
#define FD_DEF_U32_DPP( name, PERM )                                                       \
FD_DEV u32 name( u32 x ) {                                                                 \
  u32 r;                                                                                   \
  asm volatile( "s_nop 1\n\t" FD_DPP_MOV( 0, 1, PERM ) : "=&v"( r ) : "v"( x ) );          \
  return r;                                                                                \
}
FD_DEF_U32_DPP( fd_pair_xchg, "quad_perm:[1,0,3,2]" )   /* value of the partner lane (lane ^ 1) */
FD_DEF_FE_DPP( fe_xchg,   "quad_perm:[1,0,3,2]" )
FD_DEF_FE_DPP( fe_bcast0, "quad_perm:[0,0,0,0]" )       /* quad lane k's value in all four lanes */
FD_DEF_FE_DPP( fe_bcast1, "quad_perm:[1,1,1,1]" )
FD_DEF_FE_DPP( fe_bcast2, "quad_perm:[2,2,2,2]" )
FD_DEF_FE_DPP( fe_bcast3, "quad_perm:[3,3,3,3]" )
FD_DEF_FE_DPP( fe_swap23, "quad_perm:[0,1,3,2]" )       /* lanes 2 and 3 trade */
FD_DEF_U32_DPP( fd_bcast0, "quad_perm:[0,0,0,0]" )
FD_DEF_U32_DPP( fd_bcast1, "quad_perm:[1,1,1,1]" )

/* Broadcast fused into the arithmetic (quad_dbl, quad_add): r = OP( quad lane k's a, this lane's b ),
   one VOP2 DPP instruction per limb (the DPP applies to src0).  v_add_u32 is
   a + b, v_subrev_u32 is b - a; limbs wrap mod 2^32 exactly as the unfused
   forms do, so every result is bit-identical to bcast-then-op. */
#define FD_DPP_OP( OP, d, a, b, PERM ) OP "_dpp %" #d ", %" #a ", %" #b " " PERM " row_mask:0xf bank_mask:0xf\n\t"
#define FD_DEF_FE_DPP_OP( name, OP, PERM )                                                     \
FD_DEV void name( fe & r, fe const & a, fe const & b ) {                                       \
  asm volatile( "s_nop 1\n\t"                                                                  \
                FD_DPP_OP( OP, 0, 10, 20, PERM ) FD_DPP_OP( OP, 1, 11, 21, PERM )              \
                FD_DPP_OP( OP, 2, 12, 22, PERM ) FD_DPP_OP( OP, 3, 13, 23, PERM )              \
                FD_DPP_OP( OP, 4, 14, 24, PERM ) FD_DPP_OP( OP, 5, 15, 25, PERM )              \
                FD_DPP_OP( OP, 6, 16, 26, PERM ) FD_DPP_OP( OP, 7, 17, 27, PERM )              \
                FD_DPP_OP( OP, 8, 18, 28, PERM ) FD_DPP_OP( OP, 9, 19, 29, PERM )              \
                : "=&v"( r.v[0] ), "=&v"( r.v[1] ), "=&v"( r.v[2] ), "=&v"( r.v[3] ), "=&v"( r.v[4] ), \
                  "=&v"( r.v[5] ), "=&v"( r.v[6] ), "=&v"( r.v[7] ), "=&v"( r.v[8] ), "=&v"( r.v[9] ) \
                : "v"( a.v[0] ), "v"( a.v[1] ), "v"( a.v[2] ), "v"( a.v[3] ), "v"( a.v[4] ),      \
                  "v"( a.v[5] ), "v"( a.v[6] ), "v"( a.v[7] ), "v"( a.v[8] ), "v"( a.v[9] ),      \
                  "v"( b.v[0] ), "v"( b.v[1] ), "v"( b.v[2] ), "v"( b.v[3] ), "v"( b.v[4] ),      \
                  "v"( b.v[5] ), "v"( b.v[6] ), "v"( b.v[7] ), "v"( b.v[8] ), "v"( b.v[9] ) );    \
}
FD_DEF_FE_DPP_OP( fe_add_q0,    "v_add_u32",    "quad_perm:[0,0,0,0]" )   /* a[0] + b */
FD_DEF_FE_DPP_OP( fe_add_q1,    "v_add_u32",    "quad_perm:[1,1,1,1]" )   /* a[1] + b */
FD_DEF_FE_DPP_OP( fe_add_q2,    "v_add_u32",    "quad_perm:[2,2,2,2]" )   /* a[2] + b */
FD_DEF_FE_DPP_OP( fe_add_q3,    "v_add_u32",    "quad_perm:[3,3,3,3]" )   /* a[3] + b */
FD_DEF_FE_DPP_OP( fe_sub_q0,    "v_sub_u32",    "quad_perm:[0,0,0,0]" )   /* a[0] - b */
FD_DEF_FE_DPP_OP( fe_sub_q1,    "v_sub_u32",    "quad_perm:[1,1,1,1]" )   /* a[1] - b */
FD_DEF_FE_DPP_OP( fe_sub_q3,    "v_sub_u32",    "quad_perm:[3,3,3,3]" )   /* a[3] - b */
/* (not v_subrev_u32_dpp: measured on gfx950, tools/dppprobe, it applies the
   lane permutation to the other operand) */

/* limb-wise bias constants of fe_sub / fe_sub4 */
FD_DEV u32 fe_twop( int i )  { return (i==0) ? 0x7ffffdau : ( (i & 1) ? 0x3fffffeu : 0x7fffffeu ); }
FD_DEV u32 fe_fourp( int i ) { return (i==0) ? 0xfffffb4u : ( (i & 1) ? 0x7fffffcu : 0xffffffcu ); }
FD_DEV void fe_addc( fe & r, fe const & a, int four ) {       /* r = a + 2p (four=0) or 4p */
#pragma unroll
  for( int i=0; i<10; i++ ) r.v[i] = a.v[i] + ( four ? fe_fourp( i ) : fe_twop( i ) );
}
FD_DEV void fe_subc( fe & r, fe const & a ) {                 /* r = a - 2p (wraps; only ever subtracted) */
#pragma unroll
  for( int i=0; i<10; i++ ) r.v[i] = a.v[i] - fe_twop( i );
}
FD_DEV void fe_csub4( fe & r, fe const & a ) {                /* r = 4p - a */
#pragma unroll
  for( int i=0; i<10; i++ ) r.v[i] = fe_fourp( i ) - a.v[i];
}

/* M-step: from completed (E, F, G, H) on both lanes to lane 0 (m0, m1) =
   (X3, T3), lane 1 (m0, m1) = (Y3, Z3); E, F, G, H T or L */
template<int FM = FD_CARRY_FOLD>
FD_DEV void pair_mstep( fe & m0, fe & m1, int h, fe const & E, fe const & F, fe const & G, fe const & H ) {
  fe u, v0, v1;
  fe_sel( u,  h, G, E );
  fe_sel( v0, h, H, F );
  fe_sel( v1, h, F, H );
  fe_mul<FM>( m0, u, v0 );
  fe_mul<FM>( m1, u, v1 );
}

/* doubling of the point held as M-step output -> completed (E,F,G,H) on
   both lanes */
template<int FM = FD_CARRY_FOLD>
FD_DEV void pair_dbl( fe & E, fe & F, fe & G, fe & H, int h, fe const & m0, fe const & m1 ) {
  fe s, a1, q0, q1, p0, p1, XX, YY, SS, ZZ, t;
  fe_xchg( s, m0 );                                  /* lane 0: Y, lane 1: X */
  fe_add( t, m0, s );                                /* X + Y */
  fe_sel( a1, h, m1, t );                            /* lane 0: X+Y, lane 1: Z */
  fe_sqr<FM>( q0, m0 );                                  /* lane 0: XX, lane 1: YY */
  fe_sqr<FM>( q1, a1 );                                  /* lane 0: SS, lane 1: ZZ */
  fe_xchg( p0, q0 ); fe_xchg( p1, q1 );
  fe_sel( XX, h, p0, q0 ); fe_sel( YY, h, q0, p0 );
  fe_sel( SS, h, p1, q1 ); fe_sel( ZZ, h, q1, p1 );
  fe_add( H, YY, XX );                               /* H = YY+XX (L) */
  fe_sub( G, YY, XX );                               /* G = YY-XX (L) */
  fe_sub4( E, SS, H ); fe_wcarry( E, E );            /* E = SS-H = 2XY */
  fe_add( t, ZZ, ZZ ); fe_sub4( F, t, G ); fe_wcarry( F, F );   /* F = 2ZZ-G */
}

/* P + Q from the M-step output; each lane passes the two coordinates of Q
   it multiplies by (lane 0: Y2+X2 and 2dT2, lane 1: Y2-X2 and Z2), already
   conditionally negated -> completed (E,F,G,H) on both lanes */
template<int FM = FD_CARRY_FOLD>
FD_DEV void pair_add( fe & E, fe & F, fe & G, fe & H, int h, fe const & m0, fe const & m1,
                      fe const & q0, fe const & q1 ) {
  fe s, a, b, u, n0, n1, x0, x1, A, B, C, D;
  fe_xchg( s, m0 );                                  /* lane 0: Y, lane 1: X */
  fe_add( a, m0, s );                                /* lane 0: X+Y          */
  fe_sub( b, m0, s );                                /* lane 1: Y-X          */
  fe_sel( u, h, b, a );
  fe_mul<FM>( n0, u, q0 );                               /* lane 0: A, lane 1: B */
  fe_mul<FM>( n1, m1, q1 );                              /* lane 0: C, lane 1: Z Z2 */
  fe_xchg( x0, n0 ); fe_xchg( x1, n1 );
  fe_sel( A, h, x0, n0 ); fe_sel( B, h, n0, x0 );
  fe_sel( C, h, x1, n1 ); fe_sel( D, h, n1, x1 );
  fe_add( D, D, D );                                 /* D = 2 Z Z2 (L) */
  fe_sub( E, A, B );                                 /* E = A-B (L) */
  fe_add( H, A, B );                                 /* H = A+B (L) */
  fe_add( G, D, C );                                 /* G = D+C (L) */
  fe_sub4( F, D, C ); fe_wcarry( F, F );             /* F = D-C (T) */
}

/* HS = 0: [k](-A) + [S]B over 64 windows, compared with R; HS = 1: the
   half-size walk (fd_gpu_lattice.h) Q = [s']B + [c0](-A) + [c1](-R) from
   the wave's top window, -A and -R added in every window, one base-point
   entry per even window ([0..32768]B / 2^120 B), Q == O at the end.
   Signatures on the slow list (FD_PEND_SLOW) are left to slowl_tail (run by fd_dsm2_kernel<.,1> after
   the walk). */
/* c = neg ? -c : c: the coordinate 2dT of a negated table entry, in the many-lane walks.  (fd_dsm4_walk
   writes it out: through this function both fd_dsm4_kernel instances compile differently.) */
FD_DEV void fe_cneg( fe & c, int neg ) { fe nc; fe_neg( nc, c ); fe_sel( c, neg, nc, c ); }

template<int FM, int HS>
FD_DEV void
fd_dsm2_walk( u32                      nsig,
                uint4 const * __restrict__ tab,
                uint4 const * __restrict__ Rxy,
                i8 const *    __restrict__ digA,
                short const * __restrict__ digB,
                uint4 const * __restrict__ btab_g,
                i8 *          __restrict__ code,
                int                        semantics,
                unsigned char const * __restrict__ pstat,
                uint4 const * __restrict__ tabR,
                i8 const *    __restrict__ digR,
                uint4 const * __restrict__ btab2,
                unsigned char const * __restrict__ htop ) {
  u32 gl = blockIdx.x * FD_WG + threadIdx.x;
  u32 s = gl >> 1;
  int h = (int)( gl & 1u );
  int wtop = 63;
  if( HS ) {
    int c = s < nsig ? result_code( code[s], pstat[2*s], pstat[2*s+1], semantics, 0 ) : FD_ED25519_ERR_SIG;
    wtop = hs_wave_top( c == FD_ED25519_SUCCESS, htop, s );
    if( c != FD_ED25519_SUCCESS ) { if( s < nsig && !h && c != FD_PEND_SLOW ) code[s] = (i8)c; return; }
  } else {
    if( s >= nsig ) return;                          /* both lanes of a pair leave together */
    int c = result_code( code[s], pstat[2*s], pstat[2*s+1], semantics, 0 );   /* fd_prep_kernel left S's check only */
    if( c != FD_ED25519_SUCCESS ) { if( !h ) code[s] = (i8)c; return; }
  }
  size_t n = nsig;

  fe m0, m1, E, F, G, H, q0, q1;
  fe one = fe_one(), zero = fe_zero();
  fe_sel( m0, h, one, zero );                        /* identity: lane 0 X=0, T=0; lane 1 Y=1, Z=1 */
  m1 = m0;
  int da = digA[ (size_t)wtop*n + s ], dr = HS ? digR[ (size_t)wtop*n + s ] : 0;
  uint4 araw[4], rraw[4], braw[4];
  int db = 0;
#pragma unroll 1
  for( int w=wtop; w>=0; w-- ) {
    {                                                /* this lane's two coordinates of the -A entry */
      int neg = da < 0, e = neg ? -da : da;
      uint4 const * b = atab_entry( tab, s, e );
      int c0 = h ^ neg;                              /* 0 YpX, 1 YmX (swapped when negated) */
      int c1 = h ? 2 : 3;                            /* lane 0 T2d, lane 1 Z */
      araw[0] = b[2*c0]; araw[1] = b[2*c0+1]; araw[2] = b[2*c1]; araw[3] = b[2*c1+1];
    }
    if( HS ) {                                       /* and of the -R entry */
      int neg = dr < 0, e = neg ? -dr : dr;
      uint4 const * b = atab_entry( tabR, s, e );
      int c0 = h ^ neg, c1 = h ? 2 : 3;
      rraw[0] = b[2*c0]; rraw[1] = b[2*c0+1]; rraw[2] = b[2*c1]; rraw[3] = b[2*c1+1];
    }
    int bw = HS ? ( !(w & 1) && w < 32 ) : !(w & 3);
    if( bw ) {
      db = HS ? digB[ (size_t)( (w>>2) + ( (w & 2) ? 8 : 0 ) )*n + s ] : digB[ (size_t)(w>>2)*n + s ];
      int neg = db < 0, e = neg ? -db : db;
      uint4 const * b = ( HS && (w & 2) ? btab2 : btab_g ) + (size_t)e*6;
      int c0 = h ^ neg;                              /* 0 ypx, 1 ymx */
      braw[0] = b[2*c0]; braw[1] = b[2*c0+1];
      if( !h ) { braw[2] = b[4]; braw[3] = b[5]; }   /* lane 0 xy2d; lane 1 Z2 = 1 */
    }
    if( w != wtop ) {
#pragma unroll 1
      for( int r=0; r<4; r++ ) { pair_dbl<FM>( E, F, G, H, h, m0, m1 ); pair_mstep<FM>( m0, m1, h, E, F, G, H ); }
    }
    fe_from_quads( q0, araw[0], araw[1] );
    fe_from_quads( q1, araw[2], araw[3] );
    fe_cneg( q1, !h && da < 0 );
    pair_add<FM>( E, F, G, H, h, m0, m1, q0, q1 );
    pair_mstep<FM>( m0, m1, h, E, F, G, H );
    if( HS ) {
      fe_from_quads( q0, rraw[0], rraw[1] );
      fe_from_quads( q1, rraw[2], rraw[3] );
      fe_cneg( q1, !h && dr < 0 );
      pair_add<FM>( E, F, G, H, h, m0, m1, q0, q1 );
      pair_mstep<FM>( m0, m1, h, E, F, G, H );
    }
    if( bw ) {
      fe_from_quads( q0, braw[0], braw[1] );
      if( h ) q1 = one;
      else {
        fe_from_quads( q1, braw[2], braw[3] );
        fe_cneg( q1, db < 0 );
      }
      pair_add<FM>( E, F, G, H, h, m0, m1, q0, q1 );
      pair_mstep<FM>( m0, m1, h, E, F, G, H );
    }
    if( w > 0 ) { da = digA[ (size_t)(w-1)*n + s ]; if( HS ) dr = digR[ (size_t)(w-1)*n + s ]; }
  }
  if( HS ) {
    /* Q == O: lane 0 X == 0 (m0 = X), lane 1 Y == Z (m0 = Y, m1 = Z) */
    u32 ok = h ? (u32)fe_eq( m0, m1 ) : (u32)fe_is_zero( m0 );
    ok &= fd_pair_xchg( ok );
    if( !h ) code[s] = ok ? FD_ED25519_SUCCESS : FD_ED25519_ERR_MSG;
    return;
  }
  /* fd_ed25519_point_eq_z1: lane 0 X == x_R Z, lane 1 Y == y_R Z */
  fe z, r, u;
  fe_xchg( z, m1 );
  fe_sel( z, h, m1, z );
  uint4 const * rp = Rxy + (size_t)s*4 + 2*h;
  fe_from_quads( r, rp[0], rp[1] );
  fe_mul<FM>( u, r, z );
  u32 ok = (u32)fe_eq( u, m0 );
  ok &= fd_pair_xchg( ok );
  if( !h ) code[s] = ok ? FD_ED25519_SUCCESS : FD_ED25519_ERR_MSG;
}

template<int FM, int HS>
__global__ void __launch_bounds__( FD_WG )
fd_dsm2_kernel( u32                      nsig,
                uint4 const * __restrict__ tab,
                uint4 const * __restrict__ Rxy,
                i8 const *    __restrict__ digA,
                short const * __restrict__ digB,
                uint4 const * __restrict__ btab_g,
                i8 *          __restrict__ code,
                int                        semantics,
                unsigned char const * __restrict__ pstat,
                uint4 const * __restrict__ tabR,
                i8 const *    __restrict__ digR,
                uint4 const * __restrict__ btab2,
                unsigned char const * __restrict__ htop ,
                u32 const *   __restrict__ slow,
                u32 const *   __restrict__ slow_cnt ) {
  fd_dsm2_walk<FM, HS>( nsig, tab, Rxy, digA, digB, btab_g, code, semantics, pstat, tabR, digR, btab2, htop );
  if constexpr( HS != 0 ) slowl_tail<FM>( nsig, tab, Rxy, digA, digB, btab_g, code, slow, slow_cnt, semantics, pstat );
}

/* ---- latency path: four lanes per signature -----------------------------
   The same split taken one step further for the smallest batches: the
   four lanes q = 0..3 of a DPP quad share signature s, and every
   group-law step is ONE field multiplication per lane:
     doubling    lane q squares X, Y, Z, X+Y;
     addition    lane 0 A = (Y+X)(Y2+X2), lane 1 B = (Y-X)(Y2-X2),
                 lane 2 C = T 2dT2, lane 3 D = Z Z2;
     M-step      lane q forms X3 = EF, Y3 = GH, Z3 = GF, T3 = EH,
   so after an M-step lane q holds coordinate q of the point.  Between
   steps the lanes read each other's results with quad_perm broadcasts
   (10 DPP moves per element).  Per lane and doubling: 1 S + 1 M and
   ~200 moves / adds / selects -- about 0.7x the chain of fd_dsm2_kernel
   for 2.1x the total work of fd_dsm_kernel. */

/* M-step: E, F, G, H (T or L) on all lanes -> coordinate q of the point */
template<int FM = FD_CARRY_FOLD>
FD_DEV void quad_mstep( fe & m, int q, fe const & E, fe const & F, fe const & G, fe const & H ) {
  fe u, v;
  fe_sel( u, q==0 || q==3, E, G );
  fe_sel( v, q & 1, H, F );
  fe_mul<FM>( m, u, v );
}

template<int FM = FD_CARRY_FOLD>
FD_DEV void quad_dbl( fe & E, fe & F, fe & G, fe & H, int q, fe const & m ) {
  fe y, a, sq, XX, YY, t, t2;
  fe_bcast1( y, m );
  fe_add_q0( t, m, y );                              /* X + Y */
  fe_sel( a, q==3, t, m );                           /* X, Y, Z, X+Y */
  fe_sqr<FM>( sq, a );
  fe_bcast0( XX, sq ); fe_bcast1( YY, sq );
  fe_add( H, YY, XX );                               /* H = YY+XX (L) */
  fe_sub( G, YY, XX );                               /* G = YY-XX (L) */
  fe_sub_q3( t, sq, H ); fe_addc( E, t, 1 ); fe_wcarry( E, E );   /* E = SS-H+4p = 2XY */
  fe_csub4( t, G ); fe_add_q2( t2, sq, t ); fe_add_q2( F, sq, t2 ); fe_wcarry( F, F );   /* F = 2ZZ-G+4p */
}

/* P + Q; lane q passes the coordinate of Q it multiplies by (Y2+X2,
   Y2-X2, 2dT2, Z2), already conditionally negated */
template<int FM = FD_CARRY_FOLD>
FD_DEV void quad_add( fe & E, fe & F, fe & G, fe & H, int q, fe const & m, fe const & c ) {
  fe x, w, a, b, u, n, B, C, D, D2, t;
  fe_bcast0( x, m ); fe_swap23( w, m );              /* lane 2: T, lane 3: Z */
  fe_add_q1( a, m, x );                              /* Y+X */
  fe_subc( t, x ); fe_sub_q1( b, m, t );             /* Y-(X-2p) = Y-X+2p */
  fe_sel( u, q==1, b, a );
  fe_sel( u, q>=2, w, u );
  fe_mul<FM>( n, u, c );
  fe_bcast1( B, n );
  fe_add_q0( H, n, B );                              /* H = A+B */
  fe_subc( t, B ); fe_sub_q0( E, n, t );             /* E = A-(B-2p) = A-B+2p */
  fe_bcast3( D, n ); fe_add_q3( D2, n, D );          /* D2 = 2 Z Z2 (L) */
  fe_add_q2( G, n, D2 );                             /* G = D2+C */
  fe_bcast2( C, n ); fe_sub4( F, D2, C ); fe_wcarry( F, F );        /* F = D2-C+4p */
}

template<int FM, int HS>
FD_DEV void
fd_dsm4_walk( u32                      nsig,
                uint4 const * __restrict__ tab,
                uint4 const * __restrict__ Rxy,
                i8 const *    __restrict__ digA,
                short const * __restrict__ digB,
                uint4 const * __restrict__ btab_g,
                i8 *          __restrict__ code,
                int                        semantics,
                unsigned char const * __restrict__ pstat,
                uint4 const * __restrict__ tabR,
                i8 const *    __restrict__ digR,
                uint4 const * __restrict__ btab2,
                unsigned char const * __restrict__ htop ) {
  u32 gl = blockIdx.x * FD_WG + threadIdx.x;
  u32 s = gl >> 2;
  int q = (int)( gl & 3u );
  int wtop = 63;
  if( HS ) {                                         /* (fd_dsm2_kernel's HS = 1 walk, four lanes) */
    int c = s < nsig ? result_code( code[s], pstat[2*s], pstat[2*s+1], semantics, 0 ) : FD_ED25519_ERR_SIG;
    wtop = hs_wave_top( c == FD_ED25519_SUCCESS, htop, s );
    if( c != FD_ED25519_SUCCESS ) { if( s < nsig && !q && c != FD_PEND_SLOW ) code[s] = (i8)c; return; }
  } else {
    if( s >= nsig ) return;                          /* the four lanes of a quad leave together */
    int c = result_code( code[s], pstat[2*s], pstat[2*s+1], semantics, 0 );   /* fd_prep_kernel left S's check only */
    if( c != FD_ED25519_SUCCESS ) { if( !q ) code[s] = (i8)c; return; }
  }
  size_t n = nsig;
  fe m, E, F, G, H, c;
  fe one = fe_one(), zero = fe_zero();
  fe_sel( m, q==1 || q==2, one, zero );              /* identity (0 : 1 : 1 : 0) */
  int da = digA[ (size_t)wtop*n + s ], dr = HS ? digR[ (size_t)wtop*n + s ] : 0;
  uint4 araw[2], rraw[2], braw[2];
  int db = 0;
#pragma unroll 1
  for( int w=wtop; w>=0; w-- ) {
    {                                                /* this lane's coordinate of the -A entry */
      int neg = da < 0, e = neg ? -da : da;
      int ci = q < 2 ? ( q ^ neg ) : ( q==2 ? 3 : 2 );   /* YpX / YmX (swapped when negated), T2d, Z */
      uint4 const * b = atab_entry( tab, s, e ) + 2*ci;
      araw[0] = b[0]; araw[1] = b[1];
    }
    if( HS ) {                                       /* and of the -R entry */
      int neg = dr < 0, e = neg ? -dr : dr;
      int ci = q < 2 ? ( q ^ neg ) : ( q==2 ? 3 : 2 );
      uint4 const * b = atab_entry( tabR, s, e ) + 2*ci;
      rraw[0] = b[0]; rraw[1] = b[1];
    }
    int bw = HS ? ( !(w & 1) && w < 32 ) : !(w & 3);
    if( bw ) {
      db = HS ? digB[ (size_t)( (w>>2) + ( (w & 2) ? 8 : 0 ) )*n + s ] : digB[ (size_t)(w>>2)*n + s ];
      int neg = db < 0, e = neg ? -db : db;
      int ci = q < 2 ? ( q ^ neg ) : 2;              /* ypx / ymx, xy2d; lane 3: Z2 = 1 */
      uint4 const * b = ( HS && (w & 2) ? btab2 : btab_g ) + (size_t)e*6 + 2*ci;
      if( q < 3 ) { braw[0] = b[0]; braw[1] = b[1]; }
    }
    if( w != wtop ) {
#pragma unroll 1
      for( int r=0; r<4; r++ ) { quad_dbl<FM>( E, F, G, H, q, m ); quad_mstep<FM>( m, q, E, F, G, H ); }
    }
    fe_from_quads( c, araw[0], araw[1] );
    { fe nc; fe_neg( nc, c ); fe_sel( c, q==2 && da < 0, nc, c ); }
    quad_add<FM>( E, F, G, H, q, m, c );
    quad_mstep<FM>( m, q, E, F, G, H );
    if( HS ) {
      fe_from_quads( c, rraw[0], rraw[1] );
      { fe nc; fe_neg( nc, c ); fe_sel( c, q==2 && dr < 0, nc, c ); }
      quad_add<FM>( E, F, G, H, q, m, c );
      quad_mstep<FM>( m, q, E, F, G, H );
    }
    if( bw ) {
      if( q == 3 ) c = one;
      else {
        fe_from_quads( c, braw[0], braw[1] );
        fe nc; fe_neg( nc, c ); fe_sel( c, q==2 && db < 0, nc, c );
      }
      quad_add<FM>( E, F, G, H, q, m, c );
      quad_mstep<FM>( m, q, E, F, G, H );
    }
    if( w > 0 ) { da = digA[ (size_t)(w-1)*n + s ]; if( HS ) dr = digR[ (size_t)(w-1)*n + s ]; }
  }
  if( HS ) {
    /* Q == O: lane 0 X == 0, lane 1 Y == Z (Z from lane 2) */
    fe z; fe_bcast2( z, m );
    u32 ok = q==0 ? (u32)fe_is_zero( m ) : ( q==1 ? (u32)fe_eq( m, z ) : 1u );
    ok = fd_bcast0( ok ) & fd_bcast1( ok );
    if( !q ) code[s] = ok ? FD_ED25519_SUCCESS : FD_ED25519_ERR_MSG;
    return;
  }
  /* fd_ed25519_point_eq_z1: lane 0 X == x_R Z, lane 1 Y == y_R Z */
  fe z, r, u;
  fe_bcast2( z, m );
  uint4 const * rp = Rxy + (size_t)s*4 + 2*( q & 1 );
  fe_from_quads( r, rp[0], rp[1] );
  fe_mul<FM>( u, r, z );
  u32 ok = (u32)fe_eq( u, m );
  ok = fd_bcast0( ok ) & fd_bcast1( ok );
  if( !q ) code[s] = ok ? FD_ED25519_SUCCESS : FD_ED25519_ERR_MSG;
}

template<int FM, int HS>
__global__ void __launch_bounds__( FD_WG )
fd_dsm4_kernel( u32                      nsig,
                uint4 const * __restrict__ tab,
                uint4 const * __restrict__ Rxy,
                i8 const *    __restrict__ digA,
                short const * __restrict__ digB,
                uint4 const * __restrict__ btab_g,
                i8 *          __restrict__ code,
                int                        semantics,
                unsigned char const * __restrict__ pstat,
                uint4 const * __restrict__ tabR,
                i8 const *    __restrict__ digR,
                uint4 const * __restrict__ btab2,
                unsigned char const * __restrict__ htop ,
                u32 const *   __restrict__ slow,
                u32 const *   __restrict__ slow_cnt ) {
  fd_dsm4_walk<FM, HS>( nsig, tab, Rxy, digA, digB, btab_g, code, semantics, pstat, tabR, digR, btab2, htop );
  if constexpr( HS != 0 ) slowl_tail<FM>( nsig, tab, Rxy, digA, digB, btab_g, code, slow, slow_cnt, semantics, pstat );
}

/* ---- latency path: eight lanes per signature (half-size walk) -------------
   For batches that leave SIMDs idle even at four lanes per signature
   (<= FD_DSM8_MAX), the half-size walk's terms are split over two quads:
   quad 0 walks [c0](-A) plus base-point digits 0-7, quad 1 [c1](-R) plus
   digits 8-15, each with all 128 doublings but one variable-base add per
   window instead of two and half the base-point adds (a shorter chain for
   more total work).  At the end quad 1's point goes to quad 0 (row_shr:4 /
   row_shl:4 moves: lanes 4-7 of each group of 8 to lanes 0-3), in cached
   form (Y+X, Y-X, 2dT, Z; one multiplication), is added to quad 0's, and
   the sum is tested for the identity.  Every lane of a group leaves
   together (result codes first, like fd_dsm4_kernel<.,1>). */
FD_DEF_FE_DPP( fe_from_upper_quad, "row_shl:4" )   /* lanes 0-3 of a group of 8 read lanes 4-7 */

template<int FM>
FD_DEV void
fd_dsm8_walk( u32                      nsig,
                uint4 const * __restrict__ tabA,
                uint4 const * __restrict__ tabR,
                i8 const *    __restrict__ digA,
                i8 const *    __restrict__ digR,
                short const * __restrict__ digB,
                uint4 const * __restrict__ btab,
                uint4 const * __restrict__ btab2,
                i8 *          __restrict__ code,
                int                        semantics,
                unsigned char const * __restrict__ pstat,
                unsigned char const * __restrict__ htop ) {
  u32 gl = blockIdx.x * FD_WG + threadIdx.x;
  u32 s = gl >> 3;
  int half = (int)( ( gl >> 2 ) & 1u ), q = (int)( gl & 3u );
  int c = s < nsig ? result_code( code[s], pstat[2*s], pstat[2*s+1], semantics, 0 ) : FD_ED25519_ERR_SIG;
  int wtop = hs_wave_top( c == FD_ED25519_SUCCESS, htop, s );
  if( c != FD_ED25519_SUCCESS ) { if( s < nsig && !half && !q && c != FD_PEND_SLOW ) code[s] = (i8)c; return; }
  size_t n = nsig;
  uint4 const * tab = half ? tabR : tabA;
  i8 const *    dig = half ? digR : digA;
  fe m, E, F, G, H, cc;
  fe one = fe_one(), zero = fe_zero();
  fe_sel( m, q==1 || q==2, one, zero );              /* identity (0 : 1 : 1 : 0) */
  int da = dig[ (size_t)wtop*n + s ];
  uint4 araw[2], braw[2];
  int db = 0;
#pragma unroll 1
  for( int w=wtop; w>=0; w-- ) {
    {                                                /* this lane's coordinate of its term's table entry */
      int neg = da < 0, e = neg ? -da : da;
      int ci = q < 2 ? ( q ^ neg ) : ( q==2 ? 3 : 2 );   /* YpX / YmX (swapped when negated), T2d, Z */
      uint4 const * b = atab_entry( tab, s, e ) + 2*ci;
      araw[0] = b[0]; araw[1] = b[1];
    }
    /* quad 0: digit j at window 4j from [0..32768]B; quad 1: digit j + 8 at window 4j + 2 from 2^120 B */
    int bw = ( w & 3 ) == 2*half && w < 32;
    if( bw ) {
      db = digB[ (size_t)( (w>>2) + 8*half )*n + s ];
      int neg = db < 0, e = neg ? -db : db;
      int ci = q < 2 ? ( q ^ neg ) : 2;              /* ypx / ymx, xy2d; lane 3: Z2 = 1 */
      uint4 const * b = ( half ? btab2 : btab ) + (size_t)e*6 + 2*ci;
      if( q < 3 ) { braw[0] = b[0]; braw[1] = b[1]; }
    }
    if( w != wtop ) {
#pragma unroll 1
      for( int r=0; r<4; r++ ) { quad_dbl<FM>( E, F, G, H, q, m ); quad_mstep<FM>( m, q, E, F, G, H ); }
    }
    fe_from_quads( cc, araw[0], araw[1] );
    fe_cneg( cc, q==2 && da < 0 );
    quad_add<FM>( E, F, G, H, q, m, cc );
    quad_mstep<FM>( m, q, E, F, G, H );
    if( bw ) {
      if( q == 3 ) cc = one;
      else {
        fe_from_quads( cc, braw[0], braw[1] );
        fe_cneg( cc, q==2 && db < 0 );
      }
      quad_add<FM>( E, F, G, H, q, m, cc );
      quad_mstep<FM>( m, q, E, F, G, H );
    }
    if( w > 0 ) da = dig[ (size_t)(w-1)*n + s ];
  }
  /* quad 1's point in cached form: lane 0 Y+X, lane 1 Y-X, lane 2 2dT, lane 3 Z */
  {
    fe x, y, t, u;
    fe_bcast0( x, m ); fe_bcast1( y, m );
    fe_add( u, y, x );
    fe_sub( t, y, x );
    fe_sel( u, q==1, t, u );
    fe d2 = fe_d2();
    fe_mul<FM>( t, m, d2 );                          /* lane 3: T 2d (lane 2 keeps Z) */
    fe_sel( u, q==2, m, u );                         /* Z on lane 2 ... */
    fe_sel( u, q==3, t, u );                         /* ... 2dT on lane 3 */
    fe_swap23( t, u );                               /* quad_add order: lane 2 2dT2, lane 3 Z2 */
    fe_sel( u, q>=2, t, u );
    fe_from_upper_quad( cc, u );                     /* quad 0 receives quad 1's */
  }
  /* all lanes take part in the moves above; quad 0 adds and tests */
  quad_add<FM>( E, F, G, H, q, m, cc );
  quad_mstep<FM>( m, q, E, F, G, H );
  fe z; fe_bcast2( z, m );
  u32 ok = q==0 ? (u32)fe_is_zero( m ) : ( q==1 ? (u32)fe_eq( m, z ) : 1u );
  ok = fd_bcast0( ok ) & fd_bcast1( ok );
  if( !half && !q ) code[s] = ok ? FD_ED25519_SUCCESS : FD_ED25519_ERR_MSG;
}

template<int FM>
__global__ void __launch_bounds__( FD_WG )
fd_dsm8_kernel( u32                      nsig,
                uint4 const * __restrict__ tabA,
                uint4 const * __restrict__ tabR,
                i8 const *    __restrict__ digA,
                i8 const *    __restrict__ digR,
                short const * __restrict__ digB,
                uint4 const * __restrict__ btab,
                uint4 const * __restrict__ btab2,
                i8 *          __restrict__ code,
                int                        semantics,
                unsigned char const * __restrict__ pstat,
                unsigned char const * __restrict__ htop ,
                uint4 const * __restrict__ Rxy,
                u32 const *   __restrict__ slow,
                u32 const *   __restrict__ slow_cnt ) {
  fd_dsm8_walk<FM>( nsig, tabA, tabR, digA, digR, digB, btab, btab2, code, semantics, pstat, htop );
  slowl_tail<FM>( nsig, tabA, Rxy, digA, digB, btab, code, slow, slow_cnt, semantics, pstat );
}

/* ---- deferred R check ----------------------------------------------------
   The signature's R is never decompressed on the common path.
   fd_dsm_kernel leaves P = [k](-A) + [S]B projective, and P's affine
   encoding is compared with the 32 bytes of R:
     fd_rprod_kernel   Montgomery's trick per 256-signature block: each lane
                       gets the product of every other Z of its block (wave
                       prefix / suffix products by lane shuffles, the 4 wave
                       totals through LDS); the block writes the product of
                       all its Z;
     fd_rinv_kernel    one inversion per block;
     fd_rcheck_kernel  1/Z = (others' product) x (block inverse), x = X/Z,
                       y = Y/Z, canonical pack, compare with R.
   Equal bytes mean R decodes to exactly P (P's encoding is canonical and
   decoding is deterministic), so checks (3) and (6) of the result-code
   procedure hold and (5), R small order, is P's.  Every
   other case -- different bytes (ERR_MSG, or a non-canonical /
   undecodable / small-order R) and the A-small-order signatures, whose
   code depends on whether R decodes -- goes through fd_rslow_kernel: the
   full decode of R and the reference's checks in order.  The inversion
   costs 1/256 of a decode per signature instead of one decode each.
   Lanes without a pending verdict carry Z = 1. */
__global__ void __launch_bounds__( FD_WG )
fd_rprod_kernel( u32 nsig, i8 const * __restrict__ code, u32 const * __restrict__ Pbuf,
                 u32 * __restrict__ Obuf, u32 * __restrict__ blk, u32 * __restrict__ slow_cnt,
                 /* the half-size path's fixed-base segment, else NULL: lane i takes the signature at
                    place i of order[], i < *ocnt (a count on the device; the grid holds the worst case, blocks
                    beyond it return at once), and P, the products and the list go by place */
                 u32 const * __restrict__ order, u32 const * __restrict__ ocnt ) {
  __shared__ fe wtot[ FD_WG/64 ];
  u32 i = blockIdx.x * FD_WG + threadIdx.x;
  if( i == 0u ) *slow_cnt = 0u;                      /* fd_rcheck_kernel's append counter for this batch */
  u32 cnt = order ? *ocnt : nsig;
  if( blockIdx.x * FD_WG >= cnt ) return;
  u32 s = ( order && i < cnt ) ? order[i] : i;
  int lane = (int)( threadIdx.x & 63u ), w = (int)( threadIdx.x >> 6 );
  size_t n = nsig;
  fe one = fe_one(), z = one;
  if( i < cnt && code[s]==FD_ED25519_SUCCESS ) fe_load_planar( z, Pbuf + 20*n + i, n );
  fe pre = z, suf = z, t;
#pragma unroll 1
  for( int d=1; d<64; d<<=1 ) {
    fe_shfl_up( t, pre, d );   fe_sel( t, lane >= d, t, one );     fe_mul( pre, pre, t );
    fe_shfl_down( t, suf, d ); fe_sel( t, lane + d < 64, t, one ); fe_mul( suf, suf, t );
  }
  fe o, e;
  fe_shfl_up( o, pre, 1 );   fe_sel( o, lane > 0, o, one );        /* Z of the lanes below */
  fe_shfl_down( e, suf, 1 ); fe_sel( e, lane < 63, e, one );       /* Z of the lanes above */
  fe_mul( o, o, e );
  if( lane == 63 ) wtot[w] = pre;
  __syncthreads();
#pragma unroll
  for( int v=0; v<FD_WG/64; v++ ) if( v != w ) { fe tv = wtot[v]; fe_mul( o, o, tv ); }
  if( i < cnt ) fe_store_planar( Obuf + i, n, o );
  if( threadIdx.x == 0 ) {
    fe b = wtot[0];
#pragma unroll
    for( int v=1; v<FD_WG/64; v++ ) { fe tv = wtot[v]; fe_mul( b, b, tv ); }
#pragma unroll
    for( int i=0; i<10; i++ ) blk[(size_t)blockIdx.x*10 + i] = b.v[i];
  }
}

__global__ void __launch_bounds__( FD_WG )
fd_rinv_kernel( u32 nblk, u32 * __restrict__ blk, u32 const * __restrict__ ocnt ) {   /* ocnt: as fd_rprod_kernel's */
  u32 b = blockIdx.x * FD_WG + threadIdx.x;
  if( b >= nblk ) return;
  if( ocnt && b * FD_WG >= *ocnt ) return;           /* (a block of fd_rprod_kernel that returned at once wrote no product) */
  fe z, r;
#pragma unroll
  for( int i=0; i<10; i++ ) z.v[i] = blk[(size_t)b*10 + i];
  fe_invert( r, z );
#pragma unroll
  for( int i=0; i<10; i++ ) blk[(size_t)b*10 + i] = r.v[i];
}

__global__ void __launch_bounds__( FD_WG )
fd_rcheck_kernel( u32 nsig, i8 * __restrict__ code, uint4 const * __restrict__ Rraw, u32 const * __restrict__ Pbuf,
                  u32 const * __restrict__ Obuf, u32 const * __restrict__ blk, u32 * __restrict__ slow,
                  u32 * __restrict__ slow_cnt,
                  /* as fd_rprod_kernel's; rstride: uint4 of Rraw per signature (2; 4 where R's bytes lie in the
                     signature's Rxy slot); preq: the code of a signature whose bytes differ */
                  u32 const * __restrict__ order, u32 const * __restrict__ ocnt, u32 rstride, int preq ) {
  __shared__ u32 nslow, base;
  u32 i = blockIdx.x * FD_WG + threadIdx.x;          /* same grid as fd_rprod_kernel: block = 256 signatures */
  u32 cnt = order ? *ocnt : nsig;
  if( blockIdx.x * FD_WG >= cnt ) return;
  u32 s = ( order && i < cnt ) ? order[i] : i;
  if( threadIdx.x == 0u ) nslow = 0u;
  __syncthreads();
  int c = i < cnt ? (int)code[s] : FD_ED25519_ERR_SIG;
  int is_slow = c == FD_PEND_ASMALL;
  if( c == FD_ED25519_SUCCESS ) {
    size_t n = nsig;
    fe o, bi, zi, X, Y, x, y;
    fe_load_planar( o, Obuf + i, n );
#pragma unroll
    for( int i=0; i<10; i++ ) bi.v[i] = blk[(size_t)blockIdx.x*10 + i];
    fe_mul( zi, o, bi );
    fe_load_planar( X, Pbuf + i, n );
    fe_load_planar( Y, Pbuf + 10*n + i, n );
    fe_mul( x, X, zi ); fe_mul( y, Y, zi );
    u32 wx[8], wy[8]; fe_pack( wx, x ); fe_pack( wy, y );
    uint4 r0 = Rraw[rstride*(size_t)s], r1 = Rraw[rstride*(size_t)s+1];
    u32 rw[8] = { r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w };
    u32 diff = ( wx[0] & 1u ) ^ ( rw[7] >> 31 );      /* sign bit = parity of x */
    rw[7] &= 0x7fffffffu;
#pragma unroll
    for( int k=0; k<8; k++ ) diff |= wy[k] ^ rw[k];
    if( diff ) is_slow = 1;
    else {
      /* R == P: fd_ed25519_affine_is_small_order on P's canonical coordinates */
      u32 const y0[8] = FD_Y0_W, y1[8] = FD_Y1_W;
      u32 zx = 0u, zy = 0u, e0 = 0u, e1 = 0u;
#pragma unroll
      for( int k=0; k<8; k++ ) { zx |= wx[k]; zy |= wy[k]; e0 |= wy[k] ^ y0[k]; e1 |= wy[k] ^ y1[k]; }
      int small = (zx==0u) | (zy==0u) | (e0==0u) | (e1==0u);
      code[s] = small ? FD_ED25519_ERR_SIG : FD_ED25519_SUCCESS;
    }
  }
  /* compact the slow signatures into one list (an LDS count per block, one
     global atomic per block that has any), so fd_rslow_kernel's decodes
     fill whole waves instead of stalling every wave that holds one */
  u32 li = 0u;
  if( is_slow ) { if( c == FD_ED25519_SUCCESS ) code[s] = (i8)preq; li = atomicAdd( &nslow, 1u ); }
  __syncthreads();
  if( threadIdx.x == 0u && nslow ) base = atomicAdd( slow_cnt, nslow );
  __syncthreads();
  if( is_slow ) slow[ base + li ] = i;
}

__global__ void __launch_bounds__( FD_WG )
fd_rslow_kernel( u32 nsig, int semantics, i8 * __restrict__ code, uint4 const * __restrict__ Rraw,
                 u32 const * __restrict__ Pbuf, u32 const * __restrict__ slow, u32 const * __restrict__ slow_cnt,
                 u32 const * __restrict__ order, u32 rstride ) {   /* as fd_rcheck_kernel's: the list names places */
  u32 i = blockIdx.x * FD_WG + threadIdx.x;
  if( i >= *slow_cnt ) return;
  u32 col = slow[i], s = order ? order[col] : col;
  int c = code[s];
  size_t n = nsig;
  uint4 r0 = Rraw[rstride*(size_t)s], r1 = Rraw[rstride*(size_t)s+1];
  u32 rw[8] = { r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w };
  ge_p3 R; int rb;
  ge_decode1( R, rb, rw );
  /* (3) R fails to decode: AVX-512 also rejects x==0 with the sign bit set */
  int rfail = semantics==FDGPU_SEMANTICS_AVX512 ? rb != 0 : rb == 1;
  int r;
  if( c == FD_PEND_ASMALL ) r = rfail ? FD_ED25519_ERR_SIG : FD_ED25519_ERR_PUBKEY;       /* (3) before (4) */
  else if( rfail || ge_affine_is_small_order( R ) ) r = FD_ED25519_ERR_SIG;               /* (3), (5) */
  else {                                                /* (6) fd_ed25519_point_eq_z1 */
    fe X, Y, Z, u;
    fe_load_planar( X, Pbuf + col, n );
    fe_load_planar( Y, Pbuf + 10*n + col, n );
    fe_load_planar( Z, Pbuf + 20*n + col, n );
    fe_mul( u, R.X, Z ); int okx = fe_eq( u, X );
    fe_mul( u, R.Y, Z ); int oky = fe_eq( u, Y );
    r = (okx & oky) ? FD_ED25519_SUCCESS : FD_ED25519_ERR_MSG;
  }
  code[s] = (i8)r;
}

/* a transaction's code from its signatures' codes: fd_ed25519_verify_batch_single_msg's order */
FD_DEV int txn_code( fdgpu_txn_desc_t const & d, u32 t, u32 nsig, i8 const * __restrict__ code,
                     unsigned char const * __restrict__ pflag ) {
  u32 cnt = d.sig_cnt;
  if( pflag && pflag[t] ) return pflag[t]==2u ? FDGPU_ERR_OVERRUN : FDGPU_ERR_PARSE;   /* fd_verify_tile.c:127-131 */
  if( cnt==0u || cnt>16u ) return FD_ED25519_ERR_SIG;         /* fd_ed25519_user.c:238-241 */
  int first = 0, any_msg = 0;
  for( u32 j=0; j<cnt; j++ ) {
    u32 s = d.sig_base + j;
    int c = s < nsig ? (int)code[s] : FD_ED25519_ERR_SIG;
    if( c==FD_ED25519_ERR_MSG ) any_msg = 1;
    else if( c && !first ) first = c;                         /* pass-1 order, :264-294 */
  }
  return first ? first : ( any_msg ? FD_ED25519_ERR_MSG : FD_ED25519_SUCCESS );   /* pass 2, :297-306 */
}

__global__ void __launch_bounds__( FD_WG )
fd_reduce_kernel( fdgpu_txn_desc_t const * __restrict__ desc, u32 txn_cnt, u32 nsig,
                  i8 const * __restrict__ code, unsigned char const * __restrict__ pflag,
                  i8 * __restrict__ txn_out ) {
  u32 t = blockIdx.x * FD_WG + threadIdx.x;
  if( t >= txn_cnt ) return;
  txn_out[t] = (i8)txn_code( desc[t], t, nsig, code, pflag );
}

struct fd_gather {             /* mode 3: copy sz bytes from src (host, device view) to arena / region offset dst */
  unsigned long src;
  unsigned int  dst;
  unsigned int  sz;            /* multiple of 16; bit 31: no write-back (the caller copies the record itself) */
  unsigned long seq_addr;      /* device view of the frag's in-mcache line seq word, 0 = no overrun check */
  unsigned long seq;           /* the seq that line held when the tile took the frag */
  unsigned long wb;            /* per-record batches (fdgpu_ed25519_submit_raw_gather_to): device view of the record's
                                  place in its own out region; 0 = the batch's region at offset dst */
};

/* The async raw batches' last work kernel (fdgpu_ed25519_submit_raw*): the reduce, then every result
   straight into the slot's pinned host arrays (device views), so no copy commands follow the batch.
   Blocks [0, tg): one thread per transaction writes its code, footprint and dedup tag (consecutive
   lanes, consecutive host addresses).  Blocks [tg, tg + ceil(n/4)): one wave per transaction copies its
   fd_txn_t image in 2-byte stores -- into the caller's out region behind the payload, with txn_t_sz in
   the record header (gathered batches), or into the slot's image array (the others).  One wave per
   image keeps every image's loads in flight at once (a block looping over its transactions' images
   waited one load latency per transaction: 80 us for a 1,536-transaction batch). */
__global__ void __launch_bounds__( FD_WG )
fd_finish_kernel( fdgpu_txn_desc_t const * __restrict__ desc, fdgpu_txn_raw_t const * __restrict__ raw, u32 txn_cnt,
                  u32 nsig, i8 const * __restrict__ code, unsigned char const * __restrict__ pflag,
                  unsigned short const * __restrict__ fp, u64 const * __restrict__ dtag,
                  unsigned char const * __restrict__ img, u32 stride,
                  i8 * __restrict__ h_out, unsigned short * __restrict__ h_fp, u64 * __restrict__ h_dtag,
                  unsigned char * __restrict__ out_region, int rec_fp_off, unsigned char * __restrict__ h_img,
                  u32 tg, unsigned char const * __restrict__ arena, fd_gather const * __restrict__ grec ) {
  if( blockIdx.x < tg ) {
    u32 t = blockIdx.x * FD_WG + threadIdx.x;
    if( t >= txn_cnt ) return;
    h_out[t] = (i8)txn_code( desc[t], t, nsig, code, pflag );
    h_fp[t] = fp[t];
    if( h_dtag ) h_dtag[t] = dtag[t];
    return;
  }
  u32 lane = threadIdx.x & 63u;
  u32 u = ( blockIdx.x - tg ) * ( FD_WG / 64u ) + ( threadIdx.x >> 6 );
  if( u >= txn_cnt ) return;
  u32 n = fp[u];
  if( !n ) return;
  unsigned char * dst;
  if( out_region || grec ) {
    fdgpu_txn_raw_t r = raw[u];
    u32 rec = r.payload_off - (u32)r._pad[0];        /* the record's offset in the arena (and in the out region) */
    /* where the record lies on the host: at rec in the batch's out region, or (per-record batches, grec) at
       its own place, which the gather record carries */
    unsigned char * rb = grec ? (unsigned char *)grec[u].wb : out_region + rec;
    dst = rb + ( ( (u32)r._pad[0] + (u32)r.payload_sz + 1u ) & ~1u );
    if( arena ) {
      /* the record's write-back into the out region, deferred from its gather to here (the gather then
         only reads over PCIe): header + payload exactly as copied at gather time -- whole 16-B pieces,
         then the tail bytes, so nothing lands where the fd_txn_t goes -- with txn_t_sz set */
      u32 end = r.payload_off + (u32)r.payload_sz - rec, n16 = end >> 4;
      uint4 const * a = (uint4 const *)( arena + rec );
      uint4 * o = (uint4 *)rb;
      uint4 w0 = make_uint4( 0u, 0u, 0u, 0u ), w1 = w0;
      if( lane < n16 ) w0 = a[lane];
      if( lane + 64u < n16 ) w1 = a[lane + 64u];
      int fix = rec_fp_off >= 0 && !( rec_fp_off & 1 ) && rec_fp_off + 2 <= 16 && n16 > 0u;
      if( fix && lane == 0u ) ((unsigned short *)&w0)[ rec_fp_off >> 1 ] = (unsigned short)n;   /* txn_t_sz */
      if( lane < n16 ) o[lane] = w0;
      if( lane + 64u < n16 ) o[lane + 64u] = w1;
      for( u32 i=lane+128u; i<n16; i+=64u ) o[i] = a[i];      /* (records past 2 KB: none from a tile) */
      for( u32 b=( n16 << 4 ) + lane; b<end; b+=64u ) rb[ b ] = arena[ rec + b ];
      if( !fix && rec_fp_off >= 0 && lane==0u ) {
        __builtin_amdgcn_s_waitcnt( 0 );                     /* (after this lane's own copy stores) */
        *(unsigned short *)( rb + (u32)rec_fp_off ) = (unsigned short)n;
      }
    } else if( rec_fp_off >= 0 && lane==0u )
      *(unsigned short *)( rb + (u32)rec_fp_off ) = (unsigned short)n;
  } else dst = h_img + (size_t)u*stride;
  unsigned short const * s16 = (unsigned short const *)( img + (size_t)u*stride );
  unsigned short v[ 7 ];                          /* up to 852 B: 426 shorts, 7 per lane, all loads first */
#pragma unroll
  for( int k=0; k<7; k++ ) { u32 i = lane + 64u*(u32)k; v[k] = i < (n >> 1) ? s16[i] : (unsigned short)0; }
#pragma unroll
  for( int k=0; k<7; k++ ) { u32 i = lane + 64u*(u32)k; if( i < (n >> 1) ) ((unsigned short *)dst)[i] = v[k]; }
  if( ( n & 1u ) && lane==0u ) dst[n-1u] = img[(size_t)u*stride + n - 1u];
}

/* Raw-payload batches: fd_txn_parse per transaction (fd_gpu_txn.h), then
   the descriptor the verify kernels consume.  A rejected payload keeps
   its reserved signature lanes (sig_lanes) but gets payload_sz = 0, so
   the decode kernel's bounds check retires those lanes at once, and its
   pflag makes the reduce kernel report FDGPU_ERR_PARSE.  A parsed
   transaction with more than 16 signatures gets sig_cnt = 0 (no lanes;
   the reduce kernel's batch-size rule gives ERR_SIG). */
/* XXH64 (the published algorithm) of the 64 bytes at p, seed: the HA
   dedup tag fd_txn_verify computes on the host, fd_hash( seed, sig0, 64 )
   (src/disco/verify/fd_verify_tile.h:79, src/util/fd_hash.c) */
#define FD_XXP1 0x9E3779B185EBCA87UL
#define FD_XXP2 0xC2B2AE3D27D4EB4FUL
#define FD_XXP3 0x165667B19E3779F9UL
#define FD_XXP4 0x85EBCA77C2B2AE63UL
FD_DEV u64 fd_rotl64( u64 x, int r ) { return (x << r) | (x >> (64 - r)); }
FD_DEV u64 fd_xxh_round( u64 acc, u64 in ) { acc += in * FD_XXP2; acc = fd_rotl64( acc, 31 ); return acc * FD_XXP1; }
FD_DEV u64 fd_xxh64_64( u64 seed, unsigned char const * p ) {
  u32 w[16];
  fd_load_words<16>( w, p );
  u64 v[4] = { seed + FD_XXP1 + FD_XXP2, seed + FD_XXP2, seed, seed - FD_XXP1 };
#pragma unroll
  for( int blk=0; blk<2; blk++ )
#pragma unroll
    for( int i=0; i<4; i++ ) v[i] = fd_xxh_round( v[i], ((u64)w[8*blk + 2*i + 1] << 32) | (u64)w[8*blk + 2*i] );
  u64 h = fd_rotl64( v[0], 1 ) + fd_rotl64( v[1], 7 ) + fd_rotl64( v[2], 12 ) + fd_rotl64( v[3], 18 );
#pragma unroll
  for( int i=0; i<4; i++ ) { h ^= fd_xxh_round( 0UL, v[i] ); h = h * FD_XXP1 + FD_XXP4; }
  h += 64UL;
  h ^= h >> 33; h *= FD_XXP2; h ^= h >> 29; h *= FD_XXP3; h ^= h >> 32;
  return h;
}

/* Half-size throughput path: each distinct public key of a batch is decoded once.  A's point, status and
   -A table depend on the 32 key bytes alone, and a batch holds far fewer keys than signatures (votes, a few
   fee payers), so one lane per signature looks its key up in an open-addressed table in HBM (ktab, a power
   of two of 32-bit slots, at least twice the batch's signatures) and the A lanes of fd_decode_kernel run
   over the representatives only.
     slot   0 = empty, else 1 + the signature that claimed it.  launch_batch clears the part of the table
            the batch uses with a memset on the stream ahead of this kernel (8 MB for 1M signatures, a few
            microseconds), so a claim is one blind compare-and-swap of 0 whose return value names the
            claimant -- no tag to read first, nothing left over from the batch before;
     probe  linear from the key's hash (XXH64's rounds over the four words, seeded per batch), at most
            `probes` slots.  Normally a lane first reads the slot with an ordinary load, so the lanes of a key
            already in the table (nearly all of them) do no atomic at all: a stale 0 only sends the lane
            to the compare-and-swap, which answers with the truth.  A taken slot names a signature whose 32
            key bytes are read back from the payload and compared -- a hash match alone never counts.  A
            lane that runs out of probes is its own representative: decoded on its own, which is what every
            lane did before, so no input makes this kernel spin or chain;
     bypass when nearly every key of a batch is distinct nothing can be saved, and a million claims cost
            0.11-0.13 ms of random accesses per 1M signatures (the key's line, the slot).  The count is known
            only after this kernel, so the verdict comes from the context's previous batch (traffic does not
            change its nature from batch to batch), through the word behind *ucnt, never through the host:
            fd_decode_kernel sets it when more than 7/8 of the signatures were representatives (below that the
            A decodes saved, 1.2 ms per 1M at none distinct, outweigh the claims).  While it
            is set only the lanes of the first FD_KD_SBLK workgroups (1/16 of the batch) look their keys up
            -- claiming blindly, without the read -- and every other lane is its own representative without
            touching its key or the table; the sample's share of representatives (ucnt[2]) decides whether
            the next batch is de-duplicated in full again.  Either way every arep[] names a lane that
            decodes that very key, so the results are the same;
     out    arep[s] = s's representative (s itself for a representative and for a malformed transaction,
            which takes no part), ulist[] = the representatives, compacted with one atomic add per
            workgroup (the waves' counts meet in LDS), *ucnt their number, and pstat[2s] = 0: with shared
            keys that byte holds only the signature's own FD_PSTAT_SLOW flag, A's status lives at
            astat[arep[s]].
   Which of a key's signatures wins its slot differs from run to run; every one of them gives the same
   point, status and table. */
#define FD_KD_PROBES 16u
/* a key's hash: XXH64's rounds over its four 64-bit words, seeded per batch */
FD_DEV u64 fd_key_hash( u32 const w[ 8 ], u32 seed32 ) {
  u64 seed = (u64)seed32 * FD_XXP3;
  u64 v0 = fd_xxh_round( seed + FD_XXP1 + FD_XXP2, ((u64)w[1] << 32) | (u64)w[0] );
  u64 v1 = fd_xxh_round( seed + FD_XXP2,           ((u64)w[3] << 32) | (u64)w[2] );
  u64 v2 = fd_xxh_round( seed,                     ((u64)w[5] << 32) | (u64)w[4] );
  u64 v3 = fd_xxh_round( seed - FD_XXP1,           ((u64)w[7] << 32) | (u64)w[6] );
  u64 h = fd_rotl64( v0, 1 ) + fd_rotl64( v1, 7 ) + fd_rotl64( v2, 12 ) + fd_rotl64( v3, 18 );
  h ^= h >> 33; h *= FD_XXP2; h ^= h >> 29; h *= FD_XXP3; h ^= h >> 32;
  return h;
}

/* The key cache: a context keeps the tables of its fixed-base keys from batch to batch.  Slot i of
   fb_cap holds a key's 32 bytes (key[8 i]), a state word (0 = empty, else the number of the batch that last used
   the slot), the number of the batch that claimed it (birth: the batch that builds its tables), the key's decode
   status (stat), and row i of fbase[] and ftab[].  A context's batches are serial on one stream, so a batch reads
   what the batch before left and nothing else moves under it. */
struct fd_kcache {
  u32 *           key;
  u32 *           state;
  u32 *           birth;
  unsigned char * stat;
  u32 *           idx;       /* this batch's index of the resident keys: 0 = empty, else 1 + slot; imask + 1 words, cleared
                                with ktab by launch_half's memset, filled by the front blocks of fd_keydedup_kernel */
  u32             imask, iprobes;
  u32             fcap;      /* slots */
  u32             batch;     /* this batch's number, never 0 */
  /* full slots */
  u32 *           full;      /* [slot] 0 = the tables j = 0 (mod 4) only, else the batch that built the other 24 */
  u32 *           plist;     /* [pmax] the slots promoted in this batch */
  u32             pmax;      /* the most slots a batch promotes (0: none, fdgpu_debug_opts_t.key_full = 1) */
  u32             fnow;      /* a claim builds all 32 tables at once (fdgpu_debug_opts_t.key_full = 2) */
  /* pinned keys */
  u32             npin;      /* slots [0, npin) hold the keys fdgpu_ed25519_set_pinned_keys named: full, never claimed */
};

template<int KS>
__global__ void __launch_bounds__( FD_WG )
fd_keydedup_kernel( unsigned char const *    __restrict__ payload,
                    fdgpu_txn_desc_t const * __restrict__ desc,
                    u32 const *              __restrict__ map,
                    u32                                   nsig,
                    u32 *                    __restrict__ ktab,
                    u32                                   kmask,
                    u32                                   seed32,
                    u32                                   probes,
                    u32 *                    __restrict__ arep,
                    u32 *                    __restrict__ ulist,
                    u32 *                    __restrict__ ucnt,
                    unsigned char *          __restrict__ pstat,
                    u32                                   sblk,
                    /* KS: the signatures per key, counted at the representative up to hot_min (launch_batch zeroes
                       kcnt[0, nsig) ahead): a plain read first and a no-return add only while below the bound, so
                       one key with a million signatures does not serialise a million atomics on one word.  The
                       bypass counts nothing: no hot and no fixed-base keys then.  hot_min is the largest bound a
                       later kernel compares with (FD_FB_MIN with fixed-base keys on).  Also zeroes the counters of
                       fd_keyclass_kernel and fd_keysplit_kernel, ucnt[3..7]. */
                    u32 *                    __restrict__ kcnt,
                    u32                                   hot_min,
                    /* the key cache (KS, fixed-base keys on; else iblk = 0): the first iblk blocks index the resident
                       keys, one lane per slot -- a slot that finds no place within the probes cannot be found in
                       this batch, and its key is then a miss, which costs a build and nothing else */
                    u32                                   iblk,
                    fd_kcache                             kc ) {
  __shared__ u32 wcnt[ FD_WG / 64 + 1 ];
  if( KS && blockIdx.x < iblk ) {
    u32 slot = blockIdx.x * FD_WG + threadIdx.x;
    /* a pinned slot is stamped with this batch's number, so that fd_keyclaim_kernel's hand passes it as it
       passes a hit, and gets its other two words back -- claimed in no batch, full -- in case launch_half's memset
       has just emptied every slot: the key, the status and the tables are not in that memset */
    if( slot < kc.npin ) { kc.state[slot] = kc.batch; kc.birth[slot] = 0u; kc.full[slot] = 1u; }
    if( slot >= kc.fcap || !kc.state[slot] ) return;
    u32 w[8];
#pragma unroll
    for( int k=0; k<8; k++ ) w[k] = kc.key[ 8u*slot + k ];
    u32 h = (u32)( fd_key_hash( w, seed32 ) >> 32 );
    for( u32 i=0; i<kc.iprobes; i++ )
      if( !atomicCAS( kc.idx + ( ( h + i ) & kc.imask ), 0u, slot + 1u ) ) break;
    return;
  }
  u32 bx = KS ? blockIdx.x - iblk : blockIdx.x;
  u32 s = bx * FD_WG + threadIdx.x;
  if( KS && !s ) {
    u32 * c = ucnt + 3;                                       /* (FD_KC_*: the three of the split, two of the fixed-base keys, */
    for( int k=0; k<5; k++ ) c[k] = 0u;                       /*  three of the key cache; the hand brought back below the slots */
    for( int k=FD_KC_HIT; k<=FD_KC_BUILD; k++ ) c[k] = 0u;    /*  so that a batch's draws never wrap, and its start noted; */
    for( int k=FD_KC_PTIX; k<=FD_KC_FWS; k++ ) c[k] = 0u;     /*  three of the full slots, two of the pinned keys, two of the wide) */
    if( iblk ) { u32 h = c[FD_KC_HAND] % kc.fcap; c[FD_KC_HAND] = h; c[FD_KC_HAND0] = h; }
  }
  int bypass = ucnt[1] != 0u;          /* (uniform: the decode kernel of the batch before wrote it) */
  int peek = !bypass;
  int own = s < nsig;
  u32 rep = s;
  if( s < nsig ) {
    pstat[2u*s] = 0u;
    u32 m = map[s];
    fdgpu_txn_desc_t d = desc[m & 0xffffffu];
    if( ( !bypass || bx < sblk ) && txn_desc_ok( d ) ) {
      u32 w[8];
      fd_load_words<8>( w, payload + d.payload_off + (u32)d.acct_addr_off + 32u*( m >> 24 ) );
      u64 h = fd_key_hash( w, seed32 );
      for( u32 i=0; i<probes; i++ ) {
        u32 * slot = ktab + ( ( (u32)h + i ) & kmask );
        u32 v = peek ? __hip_atomic_load( slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP ) : 0u;   /* an ordinary load */
        if( !v ) {
          v = atomicCAS( slot, 0u, s + 1u );
          if( !v ) break;                            /* claimed */
        }
        u32 c = v - 1u;                              /* taken: the same key? */
        if( c >= nsig ) continue;
        u32 mc = map[c];
        fdgpu_txn_desc_t dc = desc[mc & 0xffffffu];
        u32 wc[8];
        fd_load_words<8>( wc, payload + dc.payload_off + (u32)dc.acct_addr_off + 32u*( mc >> 24 ) );
        u32 diff = 0u;
#pragma unroll
        for( int k=0; k<8; k++ ) diff |= w[k] ^ wc[k];
        if( !diff ) { rep = c; own = 0; break; }
      }
      if( KS && !bypass ) {
        u32 * kc = kcnt + rep;
        if( __hip_atomic_load( kc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP ) < hot_min ) atomicAdd( kc, 1u );
      }
    }
    arep[s] = rep;
  }
  /* the workgroup's representatives, appended with one atomic add: each wave's count to LDS, thread 0
     adds their sum, every lane takes its wave's base + its rank in the wave */
  unsigned long long mk = __ballot( own );
  u32 lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  if( !lane ) wcnt[wv] = (u32)__popcll( mk );
  __syncthreads();
  /* bypass: the lanes behind the sample are all representatives and take the list's head in order, with
     no atomic that anything waits for; the sample's follow, placed by the sample's own counter */
  u32 nsamp = sblk * FD_WG < nsig ? sblk * FD_WG : nsig;
  if( !threadIdx.x ) {
    u32 tot = 0u;
    for( u32 k=0; k<FD_WG/64; k++ ) { u32 c = wcnt[k]; wcnt[k] = tot; tot += c; }
    u32 base = 0u;
    if( !bypass ) {
      if( tot ) base = atomicAdd( ucnt, tot );
      if( tot && bx < sblk ) atomicAdd( ucnt + 2, tot );     /* the sample's representatives */
    } else if( bx < sblk ) {
      if( tot ) { base = ( nsig - nsamp ) + atomicAdd( ucnt + 2, tot ); atomicAdd( ucnt, tot ); }
      if( !bx && nsig > nsamp ) atomicAdd( ucnt, nsig - nsamp );
    }
    wcnt[ FD_WG/64 ] = base;
  }
  __syncthreads();
  if( own ) {
    if( bypass && bx >= sblk ) ulist[ s - nsamp ] = s;
    else ulist[ wcnt[ FD_WG/64 ] + wcnt[wv] + (u32)__popcll( mk & ( ( 1ULL << lane ) - 1ULL ) ) ] = s;
  }
}

/* Repeated keys, after fd_keydedup_kernel, one lane per signature.  A key is hot when its count
   reached hot_min; a signature is hot when its key is.
     hidx[rep], hlist[]  the hot representatives get a dense index (at most nsig / hot_min of them, which sizes
                         the high tables) and are listed by it;
     order[]             the hot signatures from the front, the cold ones (and the lanes of malformed
                         transactions) from the back: fd_hashh_kernel and fd_dsmh_kernel then run lane i <->
                         signature order[i] (ks_pos);
     cnt[0..2]           hot keys, hot signatures, cold signatures (zeroed by fd_keydedup_kernel).
   A ballot per wave, the waves' counts summed in LDS, one atomic add per workgroup and list, as ulist.  No lane
   reads what another lane of this launch writes. */
/* fidx (fixed-base keys; NULL: none): a signature whose key counted fb_min signatures and whose
   representative fd_keyclass_kernel gave an index is fixed-base and not hot (a batch without such a key reads no
   fidx[], and the bypass counted nothing); those fill order[] from the front (cnt[FD_KC_FB]), and the hot ones are listed
   in orderh[] instead, because where their segment of order[] starts is known only after this launch (ks_sig). */
__global__ void __launch_bounds__( FD_WG )
fd_keysplit_kernel( u32 nsig, u32 const * __restrict__ arep, u32 const * __restrict__ kcnt, u32 hot_min,
                    u32 * __restrict__ hidx, u32 * __restrict__ hlist, u32 * __restrict__ order, u32 * __restrict__ cnt,
                    u32 hcap, u32 const * __restrict__ fidx, u32 * __restrict__ orderh, u32 fb_min,
                    /* pinned keys (npin = 0: none): the caller passes fb_min = 0, because fd_keyclass_kernel
                       then wrote fidx[] for every representative and a key in a slot below npin is fixed-base
                       whatever its count; cnt[FD_KC_PINS] counts those signatures */
                    u32 npin ) {
  __shared__ u32 wc[ 5 ][ FD_WG / 64 ], base[ 5 ];
  u32 s = blockIdx.x * FD_WG + threadIdx.x;
  int in = s < nsig;
  u32 rep = in ? arep[s] : 0u;
  u32 kc = in ? kcnt[rep] : 0u;
  u32 fi = in && fidx && kc >= fb_min ? fidx[rep] : FD_FB_NONE;   /* (fidx[] is read, and was written, only for such keys) */
  int fb  = fi != FD_FB_NONE;
  int hot = !fb && kc >= hot_min;
  int f[ 5 ] = { hot && rep == s, hot, in && !hot && !fb, fb, fb && fi < npin };
  u32 lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, rank[ 4 ];
#pragma unroll
  for( int k=0; k<5; k++ ) {
    unsigned long long mk = __ballot( f[k] );
    if( !lane ) wc[k][wv] = (u32)__popcll( mk );
    if( k < 4 ) rank[k] = (u32)__popcll( mk & ( ( 1ULL << lane ) - 1ULL ) );
  }
  __syncthreads();
  if( threadIdx.x < 5u ) {
    u32 k = threadIdx.x, tot = 0u;
    for( u32 w=0; w<FD_WG/64; w++ ) { u32 c = wc[k][w]; wc[k][w] = tot; tot += c; }
    base[k] = tot ? atomicAdd( cnt + ( k < 3u ? k : k == 3u ? (u32)FD_KC_FB : (u32)FD_KC_PINS ), tot ) : 0u;
  }
  __syncthreads();
  if( f[0] ) { u32 i = base[0] + wc[0][wv] + rank[0]; if( i < hcap ) { hidx[s] = i; hlist[i] = s; } }
  if( f[1] ) ( fidx ? orderh : order )[ base[1] + wc[1][wv] + rank[1] ] = s;
  if( f[2] ) order[ nsig - 1u - ( base[2] + wc[2][wv] + rank[2] ) ] = s;
  if( f[3] ) order[ base[3] + wc[3][wv] + rank[3] ] = s;
}

/* Fixed-base keys, between fd_keydedup_kernel and fd_keysplit_kernel, one lane per representative
   (ulist[0, ucnt[0]); the grid holds the worst case, blocks beyond the count return at once): one whose key has
   fb_min signatures looks the key up among the context's resident keys (the index the launch before filled; all
   32 bytes compared, a hash match alone never counts).
     hit   the slot is stamped with this batch's number (a plain store: every writer writes the same value), which
           keeps it from this batch's claims; fidx[rep] = the slot, astat[rep] = the status the slot recorded --
           fd_decode_kernel skips this representative -- and cnt[FD_KC_FBK], cnt[FD_KC_HIT] count it;
     miss  fidx[rep] = FD_FB_NONE, and the representative joins mlist[] (one atomic add per miss: at most
           nsig / fb_min of them) for fd_keyclaim_kernel.
   fidx[rep] is written for these representatives alone: fd_keysplit_kernel reads it only where the count reached
   fb_min too.  A launch of its own, because fd_keysplit_kernel's lanes read their representative's class.  A
   batch the de-duplication only sampled (ucnt[1] set) counted nothing: no lane of this kernel does anything.
   With pinned keys (kc.npin != 0) every representative looks its key up, in a sampled batch too, and
   fidx[rep] is written for every one of them: a key found in a slot below npin is fixed-base whatever its count. */
__global__ void __launch_bounds__( FD_WG )
fd_keyclass_kernel( u32 const * __restrict__ ulist, u32 const * __restrict__ ucnt, u32 const * __restrict__ kcnt,
                    u32 fb_min, u32 * __restrict__ fidx, u32 * __restrict__ mlist, u32 * __restrict__ cnt,
                    unsigned char const * __restrict__ payload, fdgpu_txn_desc_t const * __restrict__ desc,
                    u32 const * __restrict__ map, u32 seed32, unsigned char * __restrict__ astat, fd_kcache kc ) {
  u32 i = blockIdx.x * FD_WG + threadIdx.x;
  int sampled = ucnt[1] != 0u;
  if( ( sampled && !kc.npin ) || i >= ucnt[0] ) return;
  u32 s = ulist[i];
  int bound = !sampled && kcnt[s] >= fb_min;
  if( !bound && !kc.npin ) return;
  u32 m = map[s];
  fdgpu_txn_desc_t d = desc[m & 0xffffffu];
  /* (with pins every representative comes this far, also a malformed transaction's, whose acct_addr_off may point
     outside the payload: it loads no key.  One at the bound is well-formed: the de-duplication counted it) */
  if( kc.npin && !txn_desc_ok( d ) ) { fidx[s] = FD_FB_NONE; return; }
  u32 w[8];
  fd_load_words<8>( w, payload + d.payload_off + (u32)d.acct_addr_off + 32u*( m >> 24 ) );
  u32 h = (u32)( fd_key_hash( w, seed32 ) >> 32 );
  u32 slot = FD_FB_NONE;
  for( u32 p=0; p<kc.iprobes; p++ ) {
    u32 v = kc.idx[ ( h + p ) & kc.imask ];
    if( !v ) break;                                  /* (no insert after the launch before: an empty word ends the search) */
    u32 sl = v - 1u;
    if( sl >= kc.fcap ) continue;
    u32 diff = 0u;
#pragma unroll
    for( int k=0; k<8; k++ ) diff |= w[k] ^ kc.key[ 8u*sl + k ];
    if( diff ) continue;
    if( sl < kc.npin ) {
      /* a pinned key: fixed-base whatever its count, its slot full and already stamped by the index lanes;
         it is no hit of the cache's count, promotes nothing and claims nothing */
      fidx[s] = sl;
      astat[s] = kc.stat[sl];
      atomicAdd( cnt + FD_KC_FBK, 1u ); atomicAdd( cnt + FD_KC_PINK, 1u );
      return;
    }
    slot = sl;
    /* (with pins the search goes on past an unpinned slot of this key: should the key ever be resident twice -- a
       batch whose index had no room for its pinned slot claimed another -- the pinned slot wins whenever it is found) */
    if( !kc.npin ) break;
  }
  if( bound && slot != FD_FB_NONE ) {
    kc.state[slot] = kc.batch;
    fidx[s] = slot;
    u32 stt = kc.stat[slot];
    astat[s] = (unsigned char)stt;
    atomicAdd( cnt + FD_KC_FBK, 1u ); atomicAdd( cnt + FD_KC_HIT, 1u );
    /* promotion: a hit is a key seen in an earlier batch.  A slot that has tables and is not full is
       taken by one lane (the compare-and-swap: two representatives may share a key, and a slot is built once), which
       draws a ticket; a ticket below pmax lists the slot, a later one gives the slot back for a following batch */
    if( kc.pmax && !( stt & 7u ) && !kc.full[slot] && !atomicCAS( kc.full + slot, 0u, kc.batch ) ) {
      u32 tk = atomicAdd( cnt + FD_KC_PTIX, 1u );
      if( tk < kc.pmax ) kc.plist[tk] = slot; else kc.full[slot] = 0u;
    }
    return;
  }
  fidx[s] = FD_FB_NONE;
  if( bound ) mlist[ atomicAdd( cnt + FD_KC_MISS, 1u ) ] = s;
}

/* The misses claim slots, one lane per miss; the grid holds min( nsig / fb_min, fb_cap ) lanes, blocks
   beyond the device-side count return at once, and with more misses than slots the first fb_cap of the list try.  A
   lane draws slot numbers from the hand -- atomicAdd( hand, 1 ) % fb_cap, the hand below fb_cap when the batch began
   -- and takes the first slot whose state word is not this batch's number, until the batch's draws have gone
   round all fb_cap slots.  Every hand value goes to exactly one lane and names, within a batch, a slot of its own,
   and every hit was stamped by the launch before: no claim races with a hit or with another claim, and nothing
   is compared and swapped.  The claimant writes the key, both stamps and fidx[rep], and lists (slot, rep) for
   fbase_build and fd_ftab_kernel.  A miss that finds no slot keeps FD_FB_NONE and stays hot. */
__global__ void __launch_bounds__( FD_WG )
fd_keyclaim_kernel( u32 const * __restrict__ mlist, u32 * __restrict__ cnt, u32 * __restrict__ fidx,
                    u32 * __restrict__ flist, unsigned char const * __restrict__ payload,
                    fdgpu_txn_desc_t const * __restrict__ desc, u32 const * __restrict__ map, fd_kcache kc,
                    u32 cblk, uint4 * __restrict__ fbase,
                    /* the blocks from cblk + pblk on: the 16 extra base points of the promoted slots below
                       wcap, one lane per (slot, t, r): 11 r doublings from the slot's P_4t */
                    u32 pblk, uint4 * __restrict__ wbase, u32 wcap ) {
  if( blockIdx.x >= cblk + pblk ) {
    u32 i = ( blockIdx.x - cblk - pblk ) * FD_WG + threadIdx.x;
    u32 np = cnt[FD_KC_PTIX]; np = np < kc.pmax ? np : kc.pmax;
    if( ( i >> 4 ) >= np ) return;
    u32 slot = kc.plist[ i >> 4 ];
    if( slot >= wcap ) return;
    wbase_chain( wbase, fbase, slot, i & 15u );
    return;
  }
  if( blockIdx.x >= cblk ) {
    /* the blocks after the claims' (DESIGN 18): the promoted slots' P_j for j = 4t + r, r = 1..3, one lane per
       (slot, j).  The key's A is not decoded in this batch, so the chain of 8r doublings starts from the slot's own
       P_4t, which the batch that claimed the slot left in fbase[] in cached form: (Y+X, Y-X, Z) -> (2X : 2Y : 2Z);
       a doubling reads no T.  plist[] and the ticket count are the launch before's (fd_keyclass_kernel). */
    u32 i = ( blockIdx.x - cblk ) * FD_WG + threadIdx.x;
    u32 np = cnt[FD_KC_PTIX]; np = np < kc.pmax ? np : kc.pmax;
    u32 p = i / 24u, q = i % 24u;
    if( p >= np ) return;
    u32 slot = kc.plist[p], t = q / 3u, r = q % 3u + 1u;
    ge_p3 A;
    cached_to_dbl_input( A, fbase + ( (size_t)slot * FD_FB_NT + 4u*t ) * 8 );
    fbase_chain( fbase, slot, 4u*t + r, A, 8*(int)r );
    return;
  }
  u32 i = blockIdx.x * FD_WG + threadIdx.x;
  if( i >= cnt[FD_KC_MISS] || i >= kc.fcap ) return;
  u32 s = mlist[i], hand0 = cnt[FD_KC_HAND0];
  for(;;) {
    u32 hv = atomicAdd( cnt + FD_KC_HAND, 1u );
    if( hv - hand0 >= kc.fcap ) return;
    u32 slot = hv % kc.fcap;
    if( kc.state[slot] == kc.batch ) continue;       /* a hit of this batch (claims of it are at other hand values) */
    u32 m = map[s];
    fdgpu_txn_desc_t d = desc[m & 0xffffffu];
    u32 w[8];
    fd_load_words<8>( w, payload + d.payload_off + (u32)d.acct_addr_off + 32u*( m >> 24 ) );
#pragma unroll
    for( int k=0; k<8; k++ ) kc.key[ 8u*slot + k ] = w[k];
    kc.state[slot] = kc.batch; kc.birth[slot] = kc.batch;
    kc.full[slot] = kc.fnow ? kc.batch : 0u;         /* (the tables j = 0 (mod 4) only, unless tests fill the slot) */
    fidx[s] = slot;
    u32 b = atomicAdd( cnt + FD_KC_BUILD, 1u );
    flist[2u*b] = slot; flist[2u*b+1u] = s;
    atomicAdd( cnt + FD_KC_FBK, 1u );
    return;
  }
}

/* Pinned keys: the build at fdgpu_ed25519_set_pinned_keys, outside any batch.  The host has written the m
   distinct keys of its list to key[] of slots [0, m).  32 lanes per slot: lane (slot, j) decodes the key -- each of
   the 32 for itself; a control-plane call once per epoch can afford 31 decodes that a scratch row of affine points
   would save -- and, if it decodes and is not of small order, stores P_j = [2^(8j)](-A), as fbase_build does from the
   same canonical affine point.  Lane j = 0 records the status (rc | small_order << 2, as decode_one) and lists
   (slot, slot) in flist[], so that fd_ftab_kernel, launched next with cg = 4, the slots' status as its astat[] and
   pcnt[] as its counters, builds all 32 tables of every slot. */
__global__ void __launch_bounds__( FD_WG )
fd_keypin_kernel( u32 m, u32 const * __restrict__ key, unsigned char * __restrict__ sstat, uint4 * __restrict__ fbase,
                  u32 * __restrict__ flist, u32 * __restrict__ pcnt ) {
  u32 i = blockIdx.x * FD_WG + threadIdx.x;
  if( !i ) { pcnt[FD_KC_BUILD] = m; pcnt[FD_KC_PTIX] = 0u; }
  u32 slot = i / (u32)FD_FB_NT, j = i % (u32)FD_FB_NT;
  if( slot >= m ) return;
  u32 w[8];
#pragma unroll
  for( int k=0; k<8; k++ ) w[k] = key[ 8u*slot + k ];
  ge_p3 P; int rc;
  ge_decode1( P, rc, w );
  u32 st = (u32)rc | ( (u32)ge_affine_is_small_order( P ) << 2 );
  if( !j ) { sstat[slot] = (unsigned char)st; flist[2u*slot] = slot; flist[2u*slot+1u] = slot; }
  if( st & 7u ) return;
  u32 x[8], y[8];
  fe_pack( x, P.X ); fe_pack( y, P.Y );
  ge_p3 A;
  fe_unpack( A.X, x ); fe_unpack( A.Y, y );
  A.Z = fe_one();
  fe_neg( A.X, A.X ); fe_wcarry( A.X, A.X );              /* -A */
  fe_mul( A.T, A.X, A.Y );
  fbase_chain( fbase, slot, j, A, 8*(int)j );
}

/* Wide tables of slots that are filled at once: the 16 extra base points of the slots flist[] names, 16
   lanes a slot, after their P_4t are stored -- behind fd_keypin_kernel at pin time, and behind the hash launch's
   fbase_build blocks when a claim fills its slot (fdgpu_debug_opts_t.key_full = 2).  cnt: the FD_KC_* words that hold
   the count of flist[]; stat[ flist[2k+1] ] the key's status.  A promoted slot's are built in fd_keyclaim_kernel's
   launch instead. */
__global__ void __launch_bounds__( FD_WG )
fd_wbase_kernel( u32 const * __restrict__ cnt, u32 const * __restrict__ flist, unsigned char const * __restrict__ stat,
                 uint4 const * __restrict__ fbase, uint4 * __restrict__ wbase, u32 wcap ) {
  u32 i = blockIdx.x * FD_WG + threadIdx.x;
  if( ( i >> 4 ) >= cnt[FD_KC_BUILD] ) return;
  u32 slot = flist[ 2u*( i >> 4 ) ];
  if( slot >= wcap || ( stat[ flist[ 2u*( i >> 4 ) + 1u ] ] & 7u ) ) return;
  wbase_chain( wbase, fbase, slot, i & 15u );
}

/* the HA dedup seeds of a batch (kernel argument): seed[0], or with nseed > 0 seed[ the record's seed index ]
   (the verify service's batches hold several tiles' frags, each tile with its own secure seed,
   fd_verify_tile.c:166) */
struct fd_seeds { u64 seed[ 16 ]; u32 nseed; };

__global__ void __launch_bounds__( FD_WG )
fd_parse_kernel( unsigned char const *    __restrict__ payload,
                 fdgpu_txn_raw_t const *  __restrict__ raw,
                 u32                                    txn_cnt,
                 fdgpu_txn_desc_t *       __restrict__ desc_out,
                 unsigned char *          __restrict__ pflag,
                 unsigned char *          __restrict__ img,
                 u32                                    img_stride,
                 unsigned short *         __restrict__ fp_out,
                 fd_seeds                               dseeds,
                 u64 *                    __restrict__ dtag_out,
                 unsigned char const *    __restrict__ ovr,
                 u32 *                    __restrict__ map,       /* fused fd_expand_kernel (async batches), or NULL */
                 u32                                    nsig,
                 u32 *                    __restrict__ zero_word,
                 unsigned long *          __restrict__ stamp ) {  /* fd_stamp_kernel's GPU clock, or NULL */
  u32 t = blockIdx.x * FD_WG + threadIdx.x;
  if( t == 0u ) {
    if( stamp ) __hip_atomic_store( stamp, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
    if( zero_word ) { zero_word[0] = 0u; zero_word[1] = 0u; }   /* the batch's slow-list count and its count of
                                                                   distinct keys (half-size path) */
  }
  if( t >= txn_cnt ) return;
  fdgpu_txn_raw_t r = raw[t];
  if( ovr && ovr[t] ) {        /* overrun while gathered (fd_gather_kernel): never parsed, never verified */
    if( fp_out ) fp_out[t] = 0;
    if( dtag_out ) dtag_out[t] = 0UL;
    if( !desc_out ) return;
    fdgpu_txn_desc_t d;
    d.payload_off = r.payload_off; d.sig_base = r.sig_base; d.payload_sz = 0; d.message_off = 0; d.acct_addr_off = 0;
    d.signature_off = 0; d.sig_cnt = r.sig_lanes;
    desc_out[t] = d;
    pflag[t] = 2u;
    if( map ) for( u32 j=0; j<d.sig_cnt; j++ ) { u32 s = d.sig_base + j; if( s < nsig ) map[s] = t | (j << 24); }
    return;
  }
  fd_txn_hdr h;
  u32 fp = fd_txn_parse_dev( payload + r.payload_off, (u32)r.payload_sz,
                             img ? img + (size_t)t*img_stride : (unsigned char *)0, h );
  if( fp_out ) fp_out[t] = (unsigned short)fp;
  /* the HA dedup tag of a parsed transaction (its first signature), so the
     tile's after_frag never reads the payload */
  if( dtag_out ) {
    u64 seed = dseeds.nseed ? dseeds.seed[ r._pad[1] & 15u ] : dseeds.seed[0];
    dtag_out[t] = fp ? fd_xxh64_64( seed, payload + r.payload_off + h.sig_off ) : 0UL;
  }
  if( !desc_out ) return;
  fdgpu_txn_desc_t d;
  d.payload_off = r.payload_off; d.sig_base = r.sig_base;
  u32 lanes = h.sig_cnt <= 16u ? h.sig_cnt : 0u;
  int ok = fp != 0u && lanes == (u32)r.sig_lanes;   /* lanes != sig_lanes only if the stager lied */
  if( ok ) {
    d.payload_sz = r.payload_sz; d.message_off = (unsigned short)h.msg_off; d.acct_addr_off = (unsigned short)h.acct_off;
    d.signature_off = (unsigned char)h.sig_off; d.sig_cnt = (unsigned char)lanes;
  } else {
    d.payload_sz = 0; d.message_off = 0; d.acct_addr_off = 0; d.signature_off = 0; d.sig_cnt = r.sig_lanes;
  }
  desc_out[t] = d;
  pflag[t] = ok ? 0u : 1u;
  if( map ) for( u32 j=0; j<d.sig_cnt; j++ ) { u32 s = d.sig_base + j; if( s < nsig ) map[s] = t | (j << 24); }
}

/* Batch SHA-512 (the fd_sha512_batch_* API, src/ballet/sha512/
   fd_sha512.h:234-419, one message per lane instead of 4 / 8 AVX lanes):
   hash + 64 t = SHA-512( data[ off[t], off[t]+sz[t] ) ). */
__global__ void __launch_bounds__( FD_WG )
fd_sha512_batch_kernel( unsigned char const * __restrict__ data, unsigned long const * __restrict__ off,
                        unsigned int const * __restrict__ sz, u32 cnt, uint4 * __restrict__ hash ) {
  u32 t = blockIdx.x * FD_WG + threadIdx.x;
  if( t >= cnt ) return;
  u32 h[16];
  fd_sha512_bytes( h, data + off[t], sz[t] );
  uint4 * o = hash + (size_t)t*4;
#pragma unroll
  for( int i=0; i<4; i++ ) o[i] = make_uint4( h[4*i], h[4*i+1], h[4*i+2], h[4*i+3] );
}

/* [e]B (or [e](2^dbl B)) for e in [0,FD_BTAB_ENTRIES), affine precomputed (y+x, y-x, 2dxy),
   canonical, packed 8x32.  Generated on the device at context creation
   (the GPU analogue of table/fd_curve25519_table_*.c
   fd_ed25519_base_point_wnaf_table). */
__global__ void __launch_bounds__( 256 ) fd_btab_kernel( uint4 * out, int dbl ) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if( e >= FD_BTAB_ENTRIES ) return;
  ge_p3 B; B.X = fe_Bx(); B.Y = fe_By(); B.Z = fe_one(); fe_mul( B.T, B.X, B.Y );
  /* dbl = 120: the table of 2^120 B (the half-size path's digits 8-15 of s') */
#pragma unroll 1
  for( int i=0; i<dbl; i++ ) ge_p3_dbl( B, B );
  ge_p3 acc; ge_p3_identity( acc );
#pragma unroll 1
  for( int b=FD_BWIN; b>=0; b-- ) {
    ge_p3_dbl( acc, acc );
    if( (e >> b) & 1 ) ge_p3_add( acc, acc, B );
  }
  fe zi, x, y, ypx, ymx, xy;
  fe_invert( zi, acc.Z );
  fe_mul( x, acc.X, zi ); fe_mul( y, acc.Y, zi );
  fe_add( ypx, y, x ); fe_sub( ymx, y, x ); fe_mul( xy, x, y ); fe d2 = fe_d2(); fe_mul( xy, xy, d2 );
  uint4 * o = out + e*6;
  fe_store_packed( o + 0, ypx );
  fe_store_packed( o + 2, ymx );
  fe_store_packed( o + 4, xy );
}

/* Last launch of an async batch: stores the slot's token into its
   completion flag in pinned host memory (system scope, release), after
   every earlier command of the stream -- copies included -- completed.
   The tile polls that word with a plain load instead of a HIP call per
   poll (hipEventQuery takes runtime locks every tile thread shares). */
__global__ void fd_done_kernel( unsigned long * flag, unsigned long token, unsigned long * stamp ) {
  /* stamp (pinned, may be NULL): the 100-MHz GPU clock at the batch's end (fdgpu_ed25519_phase_stats) */
  if( stamp ) __hip_atomic_store( stamp, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
  __hip_atomic_store( flag, token, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM );
}

/* the 100-MHz GPU clock when a batch's verify kernels may start (its gathers done, the stream's
   earlier batch finished): fdgpu_ed25519_phase_stats */
__global__ void fd_stamp_kernel( unsigned long * stamp ) {
  __hip_atomic_store( stamp, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
}


/* Gathered raw batches (fdgpu_ed25519_submit_raw_gather) -- the GPU side of
   the stem's during_frag copy (src/disco/stem/fd_stem.c:667-686): one
   64-lane group per record copies it, 16 B per lane, from the caller's in
   region (host memory registered with the GPU, read over PCIe) into the
   batch arena and into the record's place in the caller's out region, then
   re-reads the frag's in-mcache seq (a system-scope load, issued after
   every lane's copy loads have returned).  A changed seq means the producer
   reused the line while the record was being read: the record is flagged
   (ovr[t] = 1) and the verify kernels report FDGPU_ERR_OVERRUN for it, the
   stem's "overrun while reading" skip.  The check happens once, here; the
   copy in the out region is what after_frag publishes.
   Gathers of a context run on their own stream, ahead of the batch that
   verifies them (the tile gathers while a batch fills): every block bumps a
   device counter once its loads have returned, and the block that brings
   it to `target` stores target into the pinned word `flag`, so the host
   learns which records have been read -- and may be overwritten in the in
   region -- without a HIP call.  The flag speaks for the loads only (the
   copies' stores reach the host's out region before the batch's verdicts,
   behind its completion token), so no release fence is needed: a
   system-scope release per block wrote back the XCD's whole L2 each time,
   under the verify kernels running beside it (2x slower stream).
   FD_GATHER_RPB records per workgroup, one wave each (ctx->gather_rpb: 4 by default -- fewer, larger
   workgroups for the dispatcher and one counter atomic per group instead of per record: with the link
   in huge pages, max rate 21.7M vs 20.1M sigs/s, profiles/r04/i; 1 = fdgpu_debug_opts_t.gather_rpb). */
template<int FD_GATHER_RPB>
__global__ void __launch_bounds__( 64 * FD_GATHER_RPB )
fd_gather_kernel( fd_gather const * __restrict__ g, u32 n, unsigned char * __restrict__ arena, unsigned char * __restrict__ out,
                  unsigned char * __restrict__ ovr, unsigned long * cnt, unsigned long * flag, unsigned long target,
                  unsigned long * gtime ) {
  /* gtime (pinned): the 100-MHz GPU clock when block 0 starts and when the last block ends -- the
     engine's gather latency metric (fdgpu_ed25519_gather_stats) */
  if( blockIdx.x == 0u && threadIdx.x == 0u )
    __hip_atomic_store( gtime, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
  u32 rec = blockIdx.x * FD_GATHER_RPB + ( threadIdx.x >> 6 ), i = threadIdx.x & 63u;
  unsigned char bad = 0;
  if( rec < n ) {
  fd_gather r = g[ rec ];
  uint4 const * src = (uint4 const *)r.src;
  uint4 * a = (uint4 *)( arena + r.dst );
  uint4 * o = r.wb ? (uint4 *)r.wb : (uint4 *)( out + r.dst );   /* (per-record batches: the record's own place) */
  if( r.wb ) out = (unsigned char *)r.wb;
  if( r.sz >> 31 ) out = NULL;                              /* FDGPU_GATHER_NO_WRITEBACK: the host copies it */
  u32 n16 = ( r.sz & 0x7fffffffu ) >> 4;
  if( n16 <= 128u ) {          /* every fd_txn_m_t record (<= 80 + 1232 bytes): all loads, the re-check, then stores */
    uint4 v0 = make_uint4( 0u, 0u, 0u, 0u ), v1 = v0;
    if( i < n16 ) v0 = src[i];
    if( i + 64u < n16 ) v1 = src[i + 64u];
    if( r.seq_addr ) {
      asm volatile( "s_waitcnt vmcnt(0)" ::: "memory" );     /* the copy's loads have all returned */
      unsigned long s = __hip_atomic_load( (unsigned long *)r.seq_addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
      bad = s != r.seq;
    }
    if( i < n16 ) { a[i] = v0; if( out ) o[i] = v0; }
    if( i + 64u < n16 ) { a[i + 64u] = v1; if( out ) o[i + 64u] = v1; }
  } else {
    for( u32 j=i; j<n16; j+=64u ) { uint4 v = src[j]; a[j] = v; if( out ) o[j] = v; }
    if( r.seq_addr ) {
      asm volatile( "s_waitcnt vmcnt(0)" ::: "memory" );
      unsigned long s = __hip_atomic_load( (unsigned long *)r.seq_addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
      bad = s != r.seq;
    }
  }
  if( i == 0u ) ovr[ rec ] = bad;                        /* (lane 0 of the record's wave) */
  }
  __syncthreads();                                          /* every lane of every wave: its loads have returned */
  if( threadIdx.x == 0u ) {
    unsigned long k = n - blockIdx.x * FD_GATHER_RPB < FD_GATHER_RPB ? n - blockIdx.x * FD_GATHER_RPB : FD_GATHER_RPB;
    unsigned long old = __hip_atomic_fetch_add( cnt, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
    if( old + k == target ) {
      __hip_atomic_store( gtime + 1, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
      __hip_atomic_store( flag, target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
    }
  }
}

/* Gathered raw batches: the fd_txn_t image of each parsed transaction
   goes straight into the caller's out region behind its payload, at the
   next 2-byte boundary (where the tile publishes it,
   fd_verify_tile.c:131-134), in 2-byte stores of one 64-lane group. */
__global__ void __launch_bounds__( 64 )
fd_img_scatter_kernel( fdgpu_txn_raw_t const * __restrict__ raw, unsigned char const * __restrict__ img, u32 stride,
                       unsigned short const * __restrict__ fp, unsigned char * __restrict__ out, int rec_fp_off ) {
  u32 t = blockIdx.x;
  u32 n = fp[t];
  fdgpu_txn_raw_t r = raw[t];
  unsigned char * dst = out + ( ( r.payload_off + (u32)r.payload_sz + 1u ) & ~1u );
  /* the footprint into the record header too (fd_txn_m_t txn_t_sz): _pad[0] = the payload's offset in its record */
  if( rec_fp_off >= 0 && threadIdx.x==0u )
    *(unsigned short *)( out + r.payload_off - (u32)r._pad[0] + (u32)rec_fp_off ) = (unsigned short)n;
  unsigned short const * s16 = (unsigned short const *)( img + (size_t)t*stride );
  for( u32 i=threadIdx.x; i<(n >> 1); i+=64u ) ((unsigned short *)dst)[i] = s16[i];
  if( ( n & 1u ) && threadIdx.x==0u ) dst[n-1u] = img[(size_t)t*stride + n - 1u];
}

/* Per-signature descriptors (fdgpu_ed25519_verify_sigs_device / _host): the records of a batch,
   named by byte offsets into the caller's arena, are packed as one-signer transactions sig | pub | msg into the
   context's pack arena, in front of an unchanged launch_batch.  fd_sig_desc.h has the validity test, the packed
   size and the placement rule, shared with the host.  Four kernels, then the batch, then fd_sig_flag_kernel:

   fd_sig_size_kernel   one lane per descriptor: its size (96 for a bad one) and flag byte, and the exclusive
                        prefix sum of the sizes inside the 256-record block; the block's total
   fd_sig_scan_kernel   one workgroup: the exclusive prefix sum of the block totals, in place, 64 bits
   fd_sig_place_kernel  one lane per record: off = block base + offset in the block; a record that ends past the
                        capacity is flagged (and with it every later one, fd_sig_desc.h); the record's
                        fdgpu_txn_desc_t
   fd_sig_pack_kernel   one wavefront per record: the copy */
#define FD_SIG_DESC_FN static inline __host__ __device__
#include "fd_sig_desc.h"

#define FD_SIG_RPB 4               /* records (wavefronts) per workgroup of fd_sig_pack_kernel, as fd_gather_kernel */

/* inclusive prefix sum over the wave's 64 lanes */
template< class T > __device__ __forceinline__ T fd_wave_scan( T x, u32 lane ) {
#pragma unroll
  for( u32 o=1u; o<64u; o<<=1 ) { T y = __shfl_up( x, o ); if( lane >= o ) x += y; }
  return x;
}

__global__ void __launch_bounds__( FD_WG )
fd_sig_size_kernel( fdgpu_sig_desc_t const * __restrict__ desc, u32 n, unsigned long arena_sz, u32 * __restrict__ loc,
                    unsigned char * __restrict__ flag, unsigned long * __restrict__ btot ) {
  __shared__ u32 wsum[ FD_WG / 64 ];
  u32 i = blockIdx.x * FD_WG + threadIdx.x, lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  u32 sz = 0u;
  if( i < n ) {
    fdgpu_sig_desc_t d = desc[i];
    int bad;
    sz = fd_sig_desc_size( d.sig_off, d.pub_off, d.msg_off, d.msg_sz, arena_sz, &bad );
    flag[i] = (unsigned char)( bad ? FD_SIG_DESC_BAD : 0 );
  }
  u32 x = fd_wave_scan( sz, lane );                          /* (at most 256 x 65,536: no overflow in 32 bits) */
  if( lane == 63u ) wsum[w] = x;
  __syncthreads();
  u32 base = 0u;
  for( u32 k=0u; k<w; k++ ) base += wsum[k];
  if( i < n ) loc[i] = base + x - sz;
  if( threadIdx.x == FD_WG - 1u ) btot[ blockIdx.x ] = (unsigned long)( base + x );
}

__global__ void __launch_bounds__( FD_WG )
fd_sig_scan_kernel( unsigned long * __restrict__ btot, u32 nb ) {
  __shared__ unsigned long long wsum[ FD_WG / 64 ];
  u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  unsigned long long carry = 0ULL;
  for( u32 lo=0u; lo<nb; lo+=FD_WG ) {                       /* (every lane takes every turn: the barriers are uniform) */
    u32 i = lo + threadIdx.x;
    unsigned long long v = i < nb ? (unsigned long long)btot[i] : 0ULL;
    unsigned long long x = fd_wave_scan( v, lane );
    if( lane == 63u ) wsum[w] = x;
    __syncthreads();
    unsigned long long base = carry, all = 0ULL;
    for( u32 k=0u; k<FD_WG/64; k++ ) { if( k < w ) base += wsum[k]; all += wsum[k]; }
    if( i < nb ) btot[i] = (unsigned long)( base + x - v );
    carry += all;
    __syncthreads();                                          /* wsum is written again next turn */
  }
}

__global__ void __launch_bounds__( FD_WG )
fd_sig_place_kernel( fdgpu_sig_desc_t const * __restrict__ desc, u32 n, u32 const * __restrict__ loc,
                     unsigned long const * __restrict__ btot, unsigned long cap, unsigned char * __restrict__ flag,
                     fdgpu_txn_desc_t * __restrict__ tdesc ) {
  u32 i = blockIdx.x * FD_WG + threadIdx.x;
  if( i >= n ) return;
  u32 f = flag[i];
  u32 msg_sz = f ? 0u : desc[i].msg_sz;                      /* (a bad record: 96 zero bytes, an empty message) */
  u32 sz = ( FD_SIG_DESC_HDR + msg_sz + 7u ) & ~7u;
  unsigned long off = btot[ blockIdx.x ] + (unsigned long)loc[i];
  int over = fd_sig_desc_over( off, sz, cap );
  if( over ) flag[i] = (unsigned char)( f | FD_SIG_DESC_OVER );
  fdgpu_txn_desc_t t;
  t.payload_off   = over ? (u32)cap : (u32)off;              /* over: not copied; the 96 zero bytes behind the capacity */
  t.sig_base      = i;
  t.payload_sz    = (unsigned short)( over ? FD_SIG_DESC_HDR : FD_SIG_DESC_HDR + msg_sz );
  t.message_off   = 96; t.acct_addr_off = 64; t.signature_off = 0; t.sig_cnt = 1;
  tdesc[i] = t;
}

/* Destination dword j of a record (0-15 the signature, 16-23 the key, then the message), from source bytes of
   any alignment: the aligned dword that holds its first byte, the next one from the lane above (which loaded it
   as its own first, when it copies the same range) or by a load of its own, and a byte-align shift.  Every
   load is an aligned dword that holds at least one byte of the range the descriptor names, so none leaves the
   arena's own dwords.  Called by all 64 lanes together (act = 0: nothing loaded, 0 returned). */
__device__ __forceinline__ u32
fd_sig_fetch( unsigned long arena, fdgpu_sig_desc_t const & d, u32 j, u32 nd, u32 lane, int act ) {
  unsigned long s; u32 last, need = 4u;
  if(      j < 16u ) { s = arena + d.sig_off + 4u * j;                          last = j == 15u; }
  else if( j < 24u ) { s = arena + d.pub_off + 4u * ( j - 16u );                last = j == 23u; }
  else               { s = arena + d.msg_off + 4UL * (unsigned long)( j - 24u ); last = j + 1u == nd;
                       if( last && ( d.msg_sz & 3u ) ) need = d.msg_sz & 3u; }
  u32 sh = (u32)s & 3u;
  u32 const * p = (u32 const *)( s & ~3UL );
  u32 lo = act ? p[0] : 0u;
  u32 hi = __shfl_down( lo, 1 );
  if( act && ( last || lane == 63u ) ) hi = sh + need > 4u ? p[1] : 0u;
  u32 v = __builtin_amdgcn_alignbyte( hi, lo, sh );
  if( need < 4u ) v &= ( 1u << ( 8u * need ) ) - 1u;         /* the message's last bytes: the padding is zero */
  return act ? v : 0u;
}

__global__ void __launch_bounds__( 64 * FD_SIG_RPB )
fd_sig_pack_kernel( unsigned char const * __restrict__ arena, fdgpu_sig_desc_t const * __restrict__ desc,
                    fdgpu_txn_desc_t const * __restrict__ tdesc, unsigned char const * __restrict__ flag, u32 n,
                    unsigned char * __restrict__ pack ) {
  u32 rec = blockIdx.x * FD_SIG_RPB + ( threadIdx.x >> 6 ), lane = threadIdx.x & 63u;
  if( rec >= n ) return;                                      /* (wave-uniform, as everything up to the copy) */
  u32 f = flag[ rec ];
  if( f & FD_SIG_DESC_OVER ) return;
  u32 * dst = (u32 *)( pack + tdesc[ rec ].payload_off );
  if( f ) { if( lane < 24u ) dst[ lane ] = 0u; return; }
  fdgpu_sig_desc_t d = desc[ rec ];
  u32 nd = 24u + ( ( d.msg_sz + 3u ) >> 2 );                  /* dwords that hold bytes of the record */
  u32 ns = 24u + ( ( ( d.msg_sz + 7u ) >> 3 ) << 1 );         /* dwords stored: the size, a multiple of 8 bytes */
  /* 1 KiB a turn: four loads in flight per lane, then four stores of 256 contiguous bytes each */
  for( u32 j0=0u; j0<ns; j0+=256u ) {
    u32 v[ 4 ];
#pragma unroll
    for( u32 k=0u; k<4u; k++ ) { u32 j = j0 + 64u * k + lane; v[k] = fd_sig_fetch( (unsigned long)arena, d, j, nd, lane, j < nd ); }
#pragma unroll
    for( u32 k=0u; k<4u; k++ ) { u32 j = j0 + 64u * k + lane; if( j < ns ) dst[j] = v[k]; }
  }
}

/* behind the batch's reduce: a flagged record's code */
__global__ void __launch_bounds__( FD_WG )
fd_sig_flag_kernel( unsigned char const * __restrict__ flag, u32 n, i8 * __restrict__ out ) {
  u32 i = blockIdx.x * FD_WG + threadIdx.x;
  if( i < n && flag[i] ) out[i] = (i8)FDGPU_ERR_DESC;
}

/* Batch SHA-256, the sibling of fd_sha512_batch_kernel: hash + 32 t = SHA-256( data[ off[t], off[t]+sz[t] ) ) */
__global__ void __launch_bounds__( FD_WG )
fd_sha256_batch_kernel( unsigned char const * __restrict__ data, unsigned long const * __restrict__ off,
                        unsigned int const * __restrict__ sz, u32 cnt, uint4 * __restrict__ hash ) {
  u32 t = blockIdx.x * FD_WG + threadIdx.x;
  if( t >= cnt ) return;
  u32 h[8];
  fd_sha256_bytes( h, data + off[t], sz[t] );
  uint4 * o = hash + (size_t)t*2;
#pragma unroll
  for( int i=0; i<2; i++ ) o[i] = make_uint4( fd_bswap32( h[4*i] ), fd_bswap32( h[4*i+1] ), fd_bswap32( h[4*i+2] ), fd_bswap32( h[4*i+3] ) );
}

/* Merkle shreds (fdgpu_ed25519_verify_shreds_device / _host): the message a shred's leader signed is
   the root of its FEC set's Merkle tree, which a verifier derives from the shred and the proof it carries.
   fd_shred_desc.h has the rules that decide a record's code before any hashing, shared with the host.  Three
   kernels around an unchanged launch_batch over the batch's sig_cnt signature slots:

   fd_shred_slot_kernel  one lane per signature slot: 128 zero bytes at pack + 128 s and the slot's
                         fdgpu_txn_desc_t, a one-signer transaction of 96 bytes with an empty message -- what a
                         slot is if no good record names it (the form fd_sig_place_kernel gives a bad record)
   fd_shred_root_kernel  one lane per record: the code of the descriptor, parse and Merkle rules; for a good
                         record the leaf (fd_sha256_shred_leaf: 15-19 blocks read where the shred lies) and one
                         merge per proof node (two blocks, the second made in registers), the root to root + 32 i,
                         and, if it names a key, sig | key | root to its slot with payload_sz 128
   fd_shred_flag_kernel  behind the batch: out[i] = the record's flagged code, else 0 without a key, else its
                         slot's code

   No load leaves the arena and its slack: a bad descriptor loads nothing; a shred under 88 bytes loads nothing; a
   longer one loads its header fields (the dwords of [64, 92)); a parsed one has sz >= 1203 or 1228 and is read to
   at most 67 bytes past that. */
#define FD_SHRED_DESC_FN static inline __host__ __device__
#include "fd_shred_desc.h"

#define FD_SHRED_SLOT 128UL        /* bytes of a signature slot of the pack: sig | key | root */

__global__ void __launch_bounds__( FD_WG )
fd_shred_slot_kernel( uint4 * __restrict__ pack, fdgpu_txn_desc_t * __restrict__ tdesc, u32 nsig ) {
  u32 s = blockIdx.x * FD_WG + threadIdx.x;
  if( s >= nsig ) return;
  uint4 * p = pack + (size_t)s * ( FD_SHRED_SLOT / 16UL );
#pragma unroll
  for( int k=0; k<8; k++ ) p[k] = make_uint4( 0u, 0u, 0u, 0u );
  fdgpu_txn_desc_t t;
  t.payload_off = (u32)( FD_SHRED_SLOT * s ); t.sig_base = s; t.payload_sz = 96;
  t.message_off = 96; t.acct_addr_off = 64; t.signature_off = 0; t.sig_cnt = 1;
  tdesc[s] = t;
}

__global__ void __launch_bounds__( FD_WG )
fd_shred_root_kernel( unsigned char const * __restrict__ arena, unsigned long arena_sz,
                      fdgpu_shred_desc_t const * __restrict__ desc, u32 n, u32 nsig,
                      uint4 const * __restrict__ keys, u32 nkey, uint4 * __restrict__ pack,
                      fdgpu_txn_desc_t * __restrict__ tdesc, i8 * __restrict__ flag, uint4 * __restrict__ root ) {
  u32 i = blockIdx.x * FD_WG + threadIdx.x;
  if( i >= n ) return;
  fdgpu_shred_desc_t d = desc[i];
  unsigned char const * sh = arena + d.off;
  fd_shred_info_t in = { 0U, 0U, 0U };
  int code;
  if( fd_shred_desc_bad( d.off, d.sz, d.key_idx, d.sig_idx, arena_sz, nkey, nsig ) ) code = FD_SHRED_ERR_DESC;
  else {
    fd_shred_fields_t f = {};
    if( d.sz >= FD_SHRED_HDR_SZ ) {
      u32 w[ FD_SHRED_FIELD_WORDS ];
      fd_load_words<FD_SHRED_FIELD_WORDS>( w, sh + 64 );
      fd_shred_fields( w, &f );
    }
    code = fd_shred_classify( &f, d.sz, d.flags, &in );
  }
  u32 h[8];
#pragma unroll
  for( int k=0; k<8; k++ ) h[k] = 0u;
  if( !code ) {
    fd_sha256_shred_leaf( h, sh + 64, in.moff - 64u );
#pragma unroll 1
    for( u32 l=0u; l<in.depth; l++ ) {
      u32 s[5];
      fd_load_words<5>( s, sh + in.moff + FD_SHRED_NODE_SZ * l );
#pragma unroll
      for( int k=0; k<5; k++ ) s[k] = fd_bswap32( s[k] );
      fd_sha256_shred_merge( h, s, (int)( ( in.leaf >> l ) & 1u ) );
    }
#pragma unroll
    for( int k=0; k<8; k++ ) h[k] = fd_bswap32( h[k] );     /* the root's bytes as little-endian words */
  }
  flag[i] = (i8)code;
  if( root ) {                                               /* (a flagged record's root: 32 zero bytes) */
    root[ 2UL*i     ] = make_uint4( h[0], h[1], h[2], h[3] );
    root[ 2UL*i+1UL ] = make_uint4( h[4], h[5], h[6], h[7] );
  }
  if( !code && d.key_idx != FD_SHRED_NO_SIG ) {
    u32 sg[16];
    fd_load_words<16>( sg, sh );
    uint4 const * k = keys + 2UL * d.key_idx;
    uint4 k0 = k[0], k1 = k[1];
    uint4 * p = pack + (size_t)d.sig_idx * ( FD_SHRED_SLOT / 16UL );
#pragma unroll
    for( int q=0; q<4; q++ ) p[q] = make_uint4( sg[4*q], sg[4*q+1], sg[4*q+2], sg[4*q+3] );
    p[4] = k0; p[5] = k1;
    p[6] = make_uint4( h[0], h[1], h[2], h[3] );
    p[7] = make_uint4( h[4], h[5], h[6], h[7] );
    fdgpu_txn_desc_t t;
    t.payload_off = (u32)( FD_SHRED_SLOT * d.sig_idx ); t.sig_base = d.sig_idx; t.payload_sz = 128;
    t.message_off = 96; t.acct_addr_off = 64; t.signature_off = 0; t.sig_cnt = 1;
    tdesc[ d.sig_idx ] = t;
  }
}

__global__ void __launch_bounds__( FD_WG )
fd_shred_flag_kernel( fdgpu_shred_desc_t const * __restrict__ desc, u32 n, i8 const * __restrict__ flag,
                      i8 const * __restrict__ code, i8 * __restrict__ out ) {
  u32 i = blockIdx.x * FD_WG + threadIdx.x;
  if( i >= n ) return;
  i8 f = flag[i];
  if( !f && desc[i].key_idx != FD_SHRED_NO_SIG ) f = code[ desc[i].sig_idx ];   /* (not flagged: sig_idx < sig_cnt) */
  out[i] = f;
}

/* FEC sets (fdgpu_ed25519_verify_fec_sets_device / _host): a complete set's whole tree -- n leaves, the
   n - 1 or so merges over them, the root and a proof for every leaf -- where fd_shred_root_kernel walks one proof
   per shred.  fd_fec_desc.h has the tree's shape and the rules that decide a set's code, shared with the host.

   fd_fec_tree_kernel  one workgroup per set, lane j its leaf j; the block is sized for the batch's largest set, so
                       lanes at or past cnt only keep the barriers.  Every loop around a barrier runs to a bound the
                       whole block shares (D, from the descriptor and the agreed code).  The device form cannot see the
                       descriptors: past the set count at which every block is resident at once it launches once per
                       block size (64, 128, 192, 256 lanes, as far as member_cnt allows) and each launch takes the sets
                       of its size, so that no set waits in a block four times its own (fec_launch).
     phase 0  each lane loads its member's header words, signature and chained root; member 0's go to LDS, the first
              code member is found with an LDS min; then every lane holds its member against them and the set's code
              (descriptor, member) is or-ed together in LDS.  A set with a code hashes nothing.
     phase 1  the leaf: fd_sha256_shred_leaf, its first 20 bytes to layer 0 in LDS
     phase 2  for l < D: barrier, lanes below ceil( n_l / 2 ) merge nodes 2j and min( 2j + 1, n_l - 1 ) into layer
              l + 1.  All layers stay: at most 510 nodes of 5 words for 256 leaves (an odd stride: a layer's stores fall
              on distinct banks; the reads at stride 10 pair up two lanes to a bank) and the root's 8 words; the LDS
              is sized by the block, 3.2 KB at 64 lanes and 11.6 KB at 256.
     phase 3  barrier; each lane compares its D proof nodes with what its shred carries (CHECK_PROOFS, not FILL),
              lane 0 the root with the expected one; barrier; then FILL lanes store their proofs where the shreds lie
              and lane 0 the root, the code and, for a keyed set, sig | key | root to its slot.
   fd_fec_flag_kernel  behind the batch: out[i] = the set's code, else 0 without a key, else its slot's code

   No load leaves the arena and its slack: a member is looked at only if off + 1203 <= arena_sz, a code shred only
   if off + 1228 <= arena_sz; the leaf reads at most 67 bytes past moff <= 1228.  Stores go to the proofs of FILL
   members of good sets only. */
#include "fd_fec_desc.h"

#define FD_FEC_WG_MAX 256
/* words of LDS a block of `lanes` lanes needs: the layers under the root (fd_fec_node_cap nodes of 5 words), the root,
   member 0 (header words, chained root, signature: 31, padded), a word per lane, three shared words (padded) */
#define FD_FEC_LDS_WORDS( lanes ) ( 5u * fd_fec_node_cap( lanes ) + 8u + 32u + (lanes) + 4u )

__global__ void __launch_bounds__( FD_FEC_WG_MAX )
fd_fec_tree_kernel( unsigned char * arena, unsigned long arena_sz, fdgpu_fec_desc_t const * __restrict__ desc,
                    fdgpu_fec_member_t const * __restrict__ member, u32 nmember, u32 nsig,
                    uint4 const * __restrict__ keys, u32 nkey, uint4 const * __restrict__ expect,
                    uint4 * __restrict__ pack, fdgpu_txn_desc_t * __restrict__ tdesc, i8 * __restrict__ flag,
                    uint4 * __restrict__ root, u32 only ) {
  extern __shared__ __attribute__(( aligned( 16 ) )) u32 fd_fec_lds[];
  u32 * node = fd_fec_lds;                                   /* the layers under the root, 5 words a node */
  u32 * top  = node + 5u * fd_fec_node_cap( blockDim.x );    /* the root */
  u32 * m0   = top + 8;                                      /* member 0: header words, chained root, signature */
  u32 * cc   = m0 + 32;                                      /* data_cnt | code_cnt << 16 as each member has them */
  u32 * sh3  = cc + blockDim.x;
  u32 & first_code = sh3[0], & st0 = sh3[1], & st1 = sh3[2];
  u32 i = blockIdx.x, j = threadIdx.x;
  fdgpu_fec_desc_t d = desc[i];
  u32 n = d.cnt;
  int set_bad = fd_fec_set_bad( d.member0, n, d.key_idx, d.sig_idx, nmember, nkey, nsig );
  /* a launch for one block size (only = lanes / 64) takes the sets that fill it, and the bad ones with the smallest:
     the whole block leaves here, in front of every barrier */
  if( only && ( set_bad ? 1u : ( n + 63u ) >> 6 ) != only ) return;
  set_bad |= n > blockDim.x;
  if( set_bad ) n = 0u;
  u32 D = n ? fd_fec_depth( n ) : 0u;

  /* phase 0 */
  if( j == 0u ) { first_code = ~0u; st0 = 0u; st1 = 0u; }
  int live = j < n, rbad = 0, cls = 1;
  fdgpu_fec_member_t m = { 0u, 0u };
  unsigned char * sh = arena;
  u32 w[ FD_SHRED_FIELD_WORDS ], ch[ 8 ], sg[ 16 ];
#pragma unroll
  for( int k=0; k<FD_SHRED_FIELD_WORDS; k++ ) w[k] = 0u;
#pragma unroll
  for( int k=0; k<8; k++ ) ch[k] = 0u;
#pragma unroll
  for( int k=0; k<16; k++ ) sg[k] = 0u;
  fd_shred_fields_t f = {};
  fd_shred_info_t in = { 0U, 0U, 0U };
  u32 type = 0u;
  if( live ) {
    m    = member[ (size_t)d.member0 + j ];
    sh   = arena + m.off;
    rbad = fd_fec_range_bad( m.off, arena_sz, 0, 0u );
    if( !rbad ) {
      fd_load_words<FD_SHRED_FIELD_WORDS>( w, sh + 64 );
      rbad = fd_fec_range_bad( m.off, arena_sz, 1, w[0] & 0xffu );
    }
    if( !rbad ) {
      fd_shred_fields( w, &f );
      type = (u32)f.variant & 0xf0u;
      cls  = fd_shred_classify( &f, fd_shred_is_code( type ) ? FD_SHRED_CODE_SZ : FD_SHRED_DATA_SZ, FD_SHRED_STRICT_LEAF, &in );
      if( !cls ) {
        fd_load_words<16>( sg, sh );
        if( fd_shred_is_chained( type ) ) fd_load_words<8>( ch, sh + in.moff - 32u );
      }
    }
  }
  __syncthreads();
  if( live ) {
    cc[j] = (u32)f.h53 | ( (u32)f.h55 << 16 );
    if( rbad ) atomicOr( &st0, 1u );
    else if( fd_shred_is_code( type ) ) atomicMin( &first_code, j );
  }
  if( j == 0u ) {
#pragma unroll
    for( int k=0; k<FD_SHRED_FIELD_WORDS; k++ ) m0[k] = w[k];
#pragma unroll
    for( int k=0; k<8; k++ ) m0[ 7+k ] = ch[k];
#pragma unroll
    for( int k=0; k<16; k++ ) m0[ 15+k ] = sg[k];
  }
  __syncthreads();
  if( live & !rbad ) {
    u32 w0[ FD_SHRED_FIELD_WORDS ], c0[ 8 ], s0[ 16 ];
#pragma unroll
    for( int k=0; k<FD_SHRED_FIELD_WORDS; k++ ) w0[k] = m0[k];
#pragma unroll
    for( int k=0; k<8; k++ ) c0[k] = m0[ 7+k ];
#pragma unroll
    for( int k=0; k<16; k++ ) s0[k] = m0[ 15+k ];
    fd_shred_fields_t f0 = {}, fc = f;
    fd_shred_fields( w0, &f0 );
    u32 fci = first_code;
    if( fci < n ) { u32 c = cc[ fci ]; fc.h53 = (unsigned short)( c & 0xffffu ); fc.h55 = (unsigned short)( c >> 16 ); }
    int bad = fd_fec_member_bad( &f, fd_fec_version( w ), &f0, fd_fec_version( w0 ), &fc, j, n, &in );
    if( !bad ) {
      if( fd_shred_is_chained( type ) ) bad = fd_fec_words_differ( ch, c0, 8U );
      bad |= fd_fec_words_differ( sg, s0, 16U );
    }
    if( bad ) atomicOr( &st0, 2u );
  }
  __syncthreads();
  u32 agreed = st0;
  int code = ( set_bad | (int)( agreed & 1u ) ) ? FD_SHRED_ERR_DESC : ( ( agreed & 2u ) ? FD_FEC_ERR_MEMBER : 0 );
  if( code ) D = 0u;                                           /* (the whole block: no merge, no proof) */

  /* phase 1 */
  if( !code && live ) {
    u32 h[8];
    fd_sha256_shred_leaf( h, sh + 64, in.moff - 64u );
#pragma unroll
    for( int k=0; k<5; k++ ) node[ 5u*j + (u32)k ] = h[k];
    if( n == 1u ) {
#pragma unroll
      for( int k=0; k<8; k++ ) top[k] = h[k];
    }
  }

  /* phase 2 */
  u32 base = 0u, nl = n;
#pragma unroll 1
  for( u32 l=0u; l<D; l++ ) {
    __syncthreads();
    u32 nn = ( nl + 1u ) >> 1;
    if( j < nn ) {
      u32 a = base + 2u*j, b = base + ( 2u*j + 1u < nl ? 2u*j + 1u : nl - 1u );
      u32 x[8], s[5];
#pragma unroll
      for( int k=0; k<5; k++ ) { x[k] = node[ 5u*a + (u32)k ]; s[k] = node[ 5u*b + (u32)k ]; }
      fd_sha256_shred_merge( x, s, 0 );
      if( l + 1u == D ) {
#pragma unroll
        for( int k=0; k<8; k++ ) top[k] = x[k];
      } else {
#pragma unroll
        for( int k=0; k<5; k++ ) node[ 5u*( base + nl + j ) + (u32)k ] = x[k];
      }
    }
    base += nl; nl = nn;
  }

  /* phase 3 */
  __syncthreads();
  int fill = ( m.flags & FD_FEC_FILL ) != 0u;
  if( !code && live && ( d.flags & FD_FEC_CHECK_PROOFS ) && !fill ) {
    u32 differ = 0u;
    base = 0u;
#pragma unroll 1
    for( u32 l=0u; l<D; l++ ) {
      u32 sib = base + fd_fec_sibling( j, l, n );
      u32 c[5];
      fd_load_words<5>( c, sh + in.moff + FD_SHRED_NODE_SZ * l );
#pragma unroll
      for( int k=0; k<5; k++ ) differ |= fd_bswap32( c[k] ) ^ node[ 5u*sib + (u32)k ];
      base += fd_fec_layer_cnt( n, l );
    }
    if( differ ) atomicOr( &st1, 2u );
  }
  u32 r[8];
#pragma unroll
  for( int k=0; k<8; k++ ) r[k] = 0u;
  if( !code && j == 0u ) {
#pragma unroll
    for( int k=0; k<8; k++ ) r[k] = fd_bswap32( top[k] );      /* the root's bytes as little-endian words */
    if( d.flags & FD_FEC_CHECK_ROOT ) {
      u32 differ = 1u;                                         /* (nothing to hold it against: not the root) */
      if( expect ) {
        uint4 e0 = expect[ 2UL*i ], e1 = expect[ 2UL*i + 1UL ];
        differ = ( e0.x ^ r[0] ) | ( e0.y ^ r[1] ) | ( e0.z ^ r[2] ) | ( e0.w ^ r[3] )
               | ( e1.x ^ r[4] ) | ( e1.y ^ r[5] ) | ( e1.z ^ r[6] ) | ( e1.w ^ r[7] );
      }
      if( differ ) atomicOr( &st1, 1u );
    }
  }
  __syncthreads();
  agreed = st1;
  if( !code ) code = ( agreed & 1u ) ? FD_FEC_ERR_ROOT : ( ( agreed & 2u ) ? FD_FEC_ERR_PROOF : 0 );
  if( !code && live && fill ) {
    base = 0u;
#pragma unroll 1
    for( u32 l=0u; l<D; l++ ) {
      u32 sib = base + fd_fec_sibling( j, l, n );
      u32 s[5];
#pragma unroll
      for( int k=0; k<5; k++ ) s[k] = node[ 5u*sib + (u32)k ];
      unsigned char * p = sh + in.moff + FD_SHRED_NODE_SZ * l;
      if( !( (uintptr_t)p & 3UL ) ) {
#pragma unroll
        for( int k=0; k<5; k++ ) ( (u32 *)p )[k] = fd_bswap32( s[k] );
      } else {
#pragma unroll
        for( int k=0; k<20; k++ ) p[k] = (unsigned char)( s[ k >> 2 ] >> ( 24 - 8*( k & 3 ) ) );
      }
      base += fd_fec_layer_cnt( n, l );
    }
  }
  if( j == 0u ) {
    flag[i] = (i8)code;
    if( root ) {                                               /* (a descriptor's or a member's code: 32 zero bytes) */
      root[ 2UL*i     ] = make_uint4( r[0], r[1], r[2], r[3] );
      root[ 2UL*i+1UL ] = make_uint4( r[4], r[5], r[6], r[7] );
    }
    if( !code && d.key_idx != FD_SHRED_NO_SIG ) {
      uint4 const * k = keys + 2UL * d.key_idx;
      uint4 k0 = k[0], k1 = k[1];
      uint4 * p = pack + (size_t)d.sig_idx * ( FD_SHRED_SLOT / 16UL );
      u32 s0[ 16 ];                                            /* (loaded again: not held through the hashes) */
      fd_load_words<16>( s0, sh );
#pragma unroll
      for( int q=0; q<4; q++ ) p[q] = make_uint4( s0[4*q], s0[4*q+1], s0[4*q+2], s0[4*q+3] );
      p[4] = k0; p[5] = k1;
      p[6] = make_uint4( r[0], r[1], r[2], r[3] );
      p[7] = make_uint4( r[4], r[5], r[6], r[7] );
      fdgpu_txn_desc_t t;
      t.payload_off = (u32)( FD_SHRED_SLOT * d.sig_idx ); t.sig_base = d.sig_idx; t.payload_sz = 128;
      t.message_off = 96; t.acct_addr_off = 64; t.signature_off = 0; t.sig_cnt = 1;
      tdesc[ d.sig_idx ] = t;
    }
  }
}

__global__ void __launch_bounds__( FD_WG )
fd_fec_flag_kernel( fdgpu_fec_desc_t const * __restrict__ desc, u32 n, i8 const * __restrict__ flag,
                    i8 const * __restrict__ code, i8 * __restrict__ out ) {
  u32 i = blockIdx.x * FD_WG + threadIdx.x;
  if( i >= n ) return;
  i8 f = flag[i];
  if( !f && desc[i].key_idx != FD_SHRED_NO_SIG ) f = code[ desc[i].sig_idx ];   /* (not flagged: sig_idx < sig_cnt) */
  out[i] = f;
}

/* ==================================================================
   Host runtime: C ABI (include/fd_ed25519_gpu.h)
   ================================================================== */

static thread_local std::string fd_err;

static unsigned long fd_now_ns( void ) {
  timespec ts; clock_gettime( CLOCK_MONOTONIC, &ts );
  return (unsigned long)ts.tv_sec * 1000000000UL + (unsigned long)ts.tv_nsec;
}
static void set_err( char const * what, hipError_t e ) {
  fd_err = std::string( what ) + ": " + hipGetErrorString( e );
}
#define HIPCHK( call, ret ) do { hipError_t _e = (call); if( _e != hipSuccess ) { set_err( #call, _e ); return ret; } } while(0)

struct fd_slot {               /* one in-flight host batch of the async pipeline */
  unsigned char *    h_payload;
  fdgpu_txn_desc_t * h_desc;   /* desc mode: fdgpu_txn_desc_t; raw mode: fdgpu_txn_raw_t (same size) */
  i8 *               h_txn_out;
  unsigned long *    h_tags;
  unsigned char *    d_payload;
  fdgpu_txn_desc_t * d_desc;
  i8 *               d_txn_out;
  unsigned short *   h_fp;     /* raw mode: footprints + fd_txn_t images (allocated on first raw use) */
  unsigned long *    h_dtag;   /* raw mode, dedup tags on: XXH64 of each parsed transaction's first signature */
  unsigned long *    d_dtag;
  unsigned char *    h_img;
  unsigned short *   d_fp;
  unsigned char *    d_img;
  size_t             payload_used;
  unsigned long      txn_cnt, sig_cnt;
  unsigned long      cursor;   /* results already handed out by poll */
  hipEvent_t         done;
  unsigned long      launch_ns;   /* host time of slot_launch, for the batch latency histogram */
  unsigned long      token;       /* value fd_done_kernel writes to the slot's completion flag */
  unsigned long      last_query;  /* host time of the last error check by hipEventQuery */
  int                state;    /* 0 filling, 1 in flight / draining */
  int                mode;     /* 0 desc (fdgpu_ed25519_submit), 1 raw (fdgpu_ed25519_submit_raw),
                                  2 raw in place (fdgpu_ed25519_submit_raw_ref),
                                  3 raw gathered by the GPU (fdgpu_ed25519_submit_raw_gather) */
  unsigned char const * ref_base; /* mode 2, 3: the caller's pinned region; payloads at [ref_lo, ref_hi) */
  size_t             ref_lo, ref_hi;
  unsigned char *    ref_dev;  /* mode 3: the device address of ref_base (the gather kernel writes the records back) */
  int                per_rec;  /* mode 3: records go back to places of their own (fdgpu_ed25519_submit_raw_gather_to;
                                  ref_base unused, arena offsets allocated in submission order) */
  struct fd_gather * h_gat;    /* mode 3: one gather record per transaction (pinned; the kernel reads it over PCIe) */
  struct fd_gather * g_dev;    /*         its device view */
  unsigned char *    d_ovr;    /*         per transaction: 1 = overrun while gathered */
  unsigned long      gathered; /*         records whose gather has been launched (fdgpu_ed25519_gather) */
  long               gt_idx;   /*         the gt[] entry timing the batch's last gather (-1: untimed) */
  /* device views of the pinned host arrays: raw batches' descriptors are read, and their results written,
     by the kernels themselves (fd_parse_kernel, fd_finish_kernel), with no copy command around the batch */
  fdgpu_txn_desc_t * hd_desc;
  i8 *               hd_txn_out;
  unsigned short *   hd_fp;
  unsigned long *    hd_dtag;
  unsigned char *    hd_img;
  unsigned long      gt_target;/*         ... and the gathered count it ends at (the entry may be reused) */
  int                path;     /* the engine path its batch ran (FDGPU_PATH_* or lanes, fdgpu_ed25519_front_batch) */
};

#define FD_NSLOT 4     /* pinned staging slots of the async pipeline */
#define FD_NRING 64    /* batches whose kernel boundaries are kept while timing is on */
#define FD_NGT   64    /* gathers timed at once */

/* A slot front-end (Merkle shreds, FEC sets): the device memory a context owns to derive a 32-byte root per record and
   have the verify batch check the signatures over the roots of the keyed ones (front_prepare) */
struct fd_front {
  unsigned long       max;       /*   records a batch may hold; 0 = unprepared */
  unsigned long       keys;      /*   keys a batch may name */
  unsigned long       sig;       /*   signature slots: min( max_sig, max_txn, max ) */
  unsigned char *     d_pack;    /*   [128 sig + 2 FD_ARENA_SLACK] the slots, sig | key | root */
  fdgpu_txn_desc_t *  d_tdesc;   /*   [sig] the slots as one-signer transactions */
  i8 *                d_code;    /*   [sig] the batch's code of each slot */
  i8 *                d_flag;    /*   [max] a record's own code, 0 = none */
  i8 *                d_out;     /*   [max] the host form's codes */
  unsigned char *     d_root;    /*   [32 max] the host form's roots */
  unsigned char *     d_keys;    /*   [32 keys] the host form's keys */
};

struct fdgpu_ed25519_ctx {
  int device, semantics, timing;
  std::vector<void *> dev_mem, pin_mem;   /* every device / pinned buffer of the context and its slots (ctx_dev_alloc,
                                             ctx_pin_alloc): what fdgpu_ed25519_ctx_delete frees */
  unsigned long max_txn, max_sig, max_payload;
  hipStream_t stream;
  hipStream_t cstream;           /* copy stream of large host batches (verify_host_pipelined) */
  hipEvent_t  pipe_ev[ FD_PIPE_MAX ];
  /* scratch */
  u32 *   d_map;
  i8 *    d_code;
  unsigned char * d_pstat;
  uint4 * d_tab;
  uint4 * d_Rxy;
  uint4 * d_Axy;
  i8 *    d_digA;
  short * d_digB;
  uint4 * d_btab;
  fdgpu_txn_desc_t * d_rdesc;    /* raw path: descriptors derived by fd_parse_kernel */
  unsigned char *    d_pflag;    /* raw path: 1 = fd_txn_parse rejected the payload */
  int dsm_lanes;                 /* latency path: lanes per signature in the DSM, 0 = by batch size (fdgpu_debug_opts_t) */
  int poll_pf;                   /* fdgpu_debug_opts_t.poll_prefetch */
  int gather_rpb;                /* fd_gather_kernel records per workgroup (fdgpu_debug_opts_t.gather_rpb) */
  int gather_cu_spread;          /* which CUs reserve_gather_cus takes (fdgpu_debug_opts_t.gather_cu_spread) */
  int gather_nowb;               /* fdgpu_debug_opts_t.gather_no_writeback: 0 = the records' write-back in
                                    the gather kernel, 1 = none (diagnostic), 2 = in fd_finish_kernel (A/B) */
  unsigned long small_max;       /* batches of at most this many signatures take the latency path */
  int last_path;                 /* the engine path launch_batch chose last (FDGPU_PATH_* or latency lanes) */
  int           excl_mode;       /* fdgpu_ed25519_set_cu_exclusive's mode; -1: off, chosen by fdgpu_debug_opts_t */
  unsigned long lat_cus;         /* fdgpu_ed25519_set_lat_share: CUs an exclusive walk may count on, 0 = no limit */
  int           quad_sha;        /* latency path: the hash role on quads up to FD_QSHA_MAX (fdgpu_debug_opts_t.quad_sha) */
  unsigned      excl_lds[ 8 ];   /* fdgpu_ed25519_set_cu_exclusive: dynamic LDS per workgroup of the latency path's
                                    prep<0,1>, prep<0,0>, dsm8, dsm4<0,1>, dsm4<0,0>, dsm2<0,1>, dsm2<0,0> (0 = none) */
  unsigned long nofold_max;      /* fd_dsm_kernel<0> (no carry fold) for batches of at most this many signatures */
  u32 *   d_P;                   /* deferred R: P = [k](-A)+[S]B, planar [30][max_sig] limbs */
  u32 *   d_O;                   /*             product of the block's other Z, planar [10][max_sig] */
  u32 *   d_blk;                 /*             per 256-signature block: product of Z, then its inverse */
  u32 *   d_slow;                /*             signatures needing R's full decode, [max_sig] + the words of slow_word
                                    (half-size path: signatures without a short (c0, c1)) */
  int     half;                  /* throughput path with half-size scalars (env FDGPU_HALF, default FD_HALF) */
  u32     half_force_slow;       /* tests: signatures with s % m == 0 take the full walk (env FDGPU_HALF_FORCE_SLOW) */
  uint4 * d_tabR;                /* half-size path: [0..8](-R), layout of d_tab */
  i8 *    d_digR;                /*                 signed radix-16 digits of c1, [FD_HDIG][max_sig] */
  unsigned char * d_htop;        /*                 highest nonzero window of c0 / c1, [max_sig] */
  uint4 * d_btab2;               /*                 [0..32768](2^120 B) */
  uint4 * d_khash;               /* NULL, or (drop-in, long messages) SHA-512(R||A||M) per signature, computed beforehand */
  int     key_dedup;             /* half-size throughput path: distinct keys decoded once.  The resolved choice, 1 = on,
                                    0 = off -- not the value of fdgpu_debug_opts_t.key_dedup (0 on, 1 off, 2 tests) */
  u32 *   d_ktab;                /*   fd_keydedup_kernel's table, kd_slots 32-bit slots (>= 2 max_sig: load <= 0.5) */
  u32     kd_slots, kd_probes;   /*   slots allocated (a power of two); probes per lane */
  int     kd_tiny;               /*   fdgpu_debug_opts_t.key_dedup = 2: every batch uses all (64) slots */
  u32     kd_seed;               /*   batches launched: the hash seed (any value is right; it only varies the probes) */
  u32 *   d_arep;                /*   [max_sig] each signature's representative */
  u32 *   d_ulist;               /*   [max_sig] the representatives + their count */
  unsigned char * d_astat;       /*   [max_sig] A's status, at the representative's index */
  int     key_split;             /* ... and the signatures of repeated keys walk 64 doublings: the resolved
                                    choice, 1 = on (needs key_dedup), 0 = off */
  u32     hot_min;               /*   signatures that make a key hot (FD_HOT_MIN; fdgpu_debug_opts_t.key_split = 2: 2) */
  u32     hot_cap;               /*   max_sig / hot_min: the most hot keys a batch can hold */
  u32 *   d_kcnt;                /*   [max_sig] signatures per key, at the representative, saturating */
  u32 *   d_hidx;                /*   [max_sig] a hot representative's dense index */
  u32 *   d_hlist;               /*   [hot_cap] the hot representatives */
  u32 *   d_order;               /*   [max_sig] hot signatures from the front, cold from the back */
  uint4 * d_htab;                /*   [hot_cap][2][8][8] the high tables, 2 KB per hot key */
  uint4 * d_btabh;               /*   [3][FD_BTAB_ENTRIES][6] [0..32768](2^e B), e = 72, 140, 196 */
  int     key_fixed;             /* ... and the keys with fb_min signatures get fixed-base tables: the resolved
                                    choice, 1 = on (needs key_split), 0 = off */
  u32     fb_min;                /*   signatures that make a key fixed-base (FD_FB_MIN; fdgpu_debug_opts_t.key_fixed = 2: 4) */
  u32     fb_cap;                /*   min( max_sig / fb_min, FD_FB_CAP ): the most fixed-base keys of a batch */
  u32 *   d_fidx;                /*   [max_sig] a fixed-base representative's slot, else FD_FB_NONE */
  u32 *   d_flist;               /*   [fb_cap][2] (slot, representative) of the keys that claimed a slot in this batch */
  /* the key cache: fb_cap slots that keep a key's fbase row and tables from batch to batch.  The
     context's batches are serial on one stream (its work buffers are shared), which is what makes this safe. */
  int     kc_mode;               /*   fdgpu_debug_opts_t.key_cache: 0 on, 1 off (every batch starts empty), 2 tests */
  int     kc_dirty;              /*   a launch failed: the next batch clears every slot first */
  u32     kc_batch;              /*   the batch number: one more per launch_half call, never 0 */
  u32     kc_iwords, kc_iprobes; /*   the per-batch index: words (a power of two, >= 4 fb_cap) in front of d_ktab; probes */
  u32 *   d_kidx;                /*   [kc_iwords] the index, then d_ktab: one memset clears both */
  u32 *   d_skey;                /*   [fb_cap][8] a slot's key */
  u32 *   d_sstate;              /*   [fb_cap] 0 = empty, else the batch that last used the slot; then [fb_cap] the batch that
                                      claimed it (d_sbirth) */
  u32 *   d_sbirth;
  u32 *   d_sfull;               /*   ... then [fb_cap] 0 = the slot has its tables j = 0 (mod 4) only, else the batch that built the
                                      other 24 */
  int     kfull_mode;            /*   fdgpu_debug_opts_t.key_full: 0 on, 1 off (no slot is ever promoted), 2 tests (a claim fills
                                      its slot at once) */
  u32     pmax;                  /*   max( 1, fb_cap / 4 ): the most slots one batch promotes; 0 with key_full off */
  u32 *   d_plist;               /*   [pmax] the slots promoted in this batch */
  u32     npin;                  /*   pinned keys (fdgpu_ed25519_set_pinned_keys): slots [0, npin) are theirs, built full
                                      at that call, stamped by every batch and so never claimed; 0: none */
  unsigned char * d_sstat;       /*   [fb_cap] the key's decode status */
  u32 *   d_mlist;               /*   [max_sig / fb_min + 1] the representatives of this batch's misses */
  u32 *   d_orderh;              /*   [max_sig] the hot signatures as the split lists them (ks_sig) */
  uint4 * d_fbase;               /*   [fb_cap][32][8] [2^(8j)](-A), cached form */
  uint4 * d_ftab;                /*   [fb_cap][32][128][6] the keys' tables, 384 KB per slot: 1.5 GiB at FD_FB_CAP */
  u32     wcap;                  /*   wide tables: slots [0, wcap) have them once full; min( fb_cap, FD_FB_WCAP ), 0 with
                                      fdgpu_debug_opts_t.key_wide = 1, fb_cap / 2 with key_wide = 2 */
  uint4 * d_wbase;               /*   [wcap][8][2][8] [2^(32t + 11r)](-A), r = 1, 2, cached form */
  uint4 * d_wtab;                /*   [6] the identity entry, then [wcap][8][FD_FB_WE][6]: 1.97 MB per slot, 1.9 GiB at FD_FB_WCAP */
  uint4 * d_btabf;               /*   [16][FD_BTAB_ENTRIES][6] [0..32768]([2^(16u)]B), 50 MB */
  u32 *   d_fslow;               /*   [max_sig] the fixed-base places whose R needs its decode (fd_rslow_kernel) */
  /* per-signature descriptors (fdgpu_ed25519_sigs_prepare): all device memory */
  unsigned long       sg_cap;    /*   the prepared size: records are packed into [0, sg_cap) of d_sg_pack; 0 = unprepared */
  unsigned char *     d_sg_pack; /*   [sg_cap + 2 FD_ARENA_SLACK] the pack arena; the bytes from sg_cap on stay zero (a record
                                      past the capacity is the 96 zero bytes there, with the slack every arena has behind it) */
  fdgpu_txn_desc_t *  d_sg_tdesc;/*   [max_sig] the records as one-signer transactions (fd_sig_place_kernel) */
  fdgpu_sig_desc_t *  d_sg_desc; /*   [max_sig] the host form's uploaded descriptors */
  u32 *               d_sg_loc;  /*   [max_sig] a record's offset inside its block of FD_WG records */
  unsigned char *     d_sg_flag; /*   [max_sig] FD_SIG_DESC_BAD | FD_SIG_DESC_OVER */
  i8 *                d_sg_out;  /*   [max_sig] the host form's codes */
  unsigned long *     d_sg_btot; /*   [max_sig / FD_WG + 1] the blocks' totals, then their prefix sum */
  /* Merkle shreds (fdgpu_ed25519_shreds_prepare): a front-end whose records are shreds, and */
  fd_front            sh;
  fdgpu_shred_desc_t * d_sh_desc;/*   [sh.max] the host form's uploaded descriptors */
  /* FEC sets (fdgpu_ed25519_fec_prepare): a front-end whose records are sets, and */
  fd_front            fc;
  unsigned long       fc_members;/*   members a batch may hold */
  unsigned long       fc_all;    /*   sets whose 256-lane blocks are all resident at once: 4 a CU (fd_fec_tree_kernel: 4 waves a SIMD) */
  fdgpu_fec_desc_t *  d_fc_desc; /*   [fc.max] the host form's uploaded descriptors */
  fdgpu_fec_member_t * d_fc_member; /* [fc_members] the host form's uploaded members */
  unsigned char *     d_fc_expect; /* [32 fc.max] the host form's expected roots */
  hipEvent_t ev[5];
  hipEvent_t ring[ FD_NRING ][ 5 ];  /* per-batch kernel boundaries while timing is on: prep start, walk start, walk end,
                                     reduce end, and (throughput path) the decode kernel's end inside the prep */
  unsigned long ring_cnt;
  /* async pipeline: FD_NSLOT pinned staging slots, all on ctx->stream */
  fd_slot slot[ FD_NSLOT ];
  int cur;                       /* slot being filled */
  int fault;                     /* a batch failed on the device: the pipeline refuses new work */
  int dbg_fail_issue;            /* test hook (fdgpu_ed25519_debug_fail_launch): the launch thread fails batch launches */
  int dedup;                     /* raw batches also return HA dedup tags (fdgpu_ed25519_set_dedup) */
  unsigned long dedup_seed;
  unsigned long dedup_seeds[ 16 ];   /* fdgpu_ed25519_set_dedup_seeds: per-record seeds (verify service) */
  int           dedup_nseed;
  int rec_fp_off;                /* gathered records: offset of a u16 footprint field, -1 = none */
  hipStream_t gstream;           /* gathered batches: the copies (fd_gather_kernel), ahead of the batch's kernels */
  hipEvent_t  gev;               /*   recorded behind a batch's last gather; the ctx stream waits for it */
  unsigned long * d_gcnt;        /*   gather blocks completed (device counter) */
  unsigned long   g_launched;    /*   records whose gather has been launched, cumulative */
  unsigned        gather_cus;    /*   CUs reserved for the gathers (fdgpu_ed25519_reserve_gather_cus), 0 = none */
  unsigned long * h_gtime;       /*   pinned [FD_NGT][2]: GPU clock (100 MHz ticks) at a gather's start / end */
  unsigned long * d_gtime;
  struct { unsigned long target, t_launch, t_issue; } gt[ FD_NGT ];   /* host side of those gathers: count they end at,
                                                                       queued ns, issued ns (the runtime call) */
  unsigned long   gt_head, gt_tail;
  double          gclk_off_ns;   /*   GPU clock ns - host CLOCK_MONOTONIC ns (calibrated once) */
  int             gclk_ok;
  unsigned long   gs_n, gs_start_sum, gs_start_max, gs_run_sum, gs_run_max;   /* fdgpu_ed25519_gather_stats */
  unsigned long   gs_issue_sum, gs_issue_max, gs_issue_slow;
  long            last_gt;       /*   gt[] entry of the last gather launched (-1: untimed) */
  unsigned long * h_stamp;       /*   pinned [FD_NSLOT][2] + 1: per slot the GPU clock when its verify kernels start
                                      (fd_stamp_kernel) and end (fd_done_kernel); [2 FD_NSLOT]: clock calibration */
  unsigned long * d_stamp;
  unsigned long   ph[ 9 ];       /*   fdgpu_ed25519_phase_stats */
  unsigned long n_batches, n_txns;                /* async batches launched, transactions in them */
  unsigned long launch_ns;                        /* host time inside slot_launch */
  unsigned long volatile * h_flag;                /* per slot: completion token written by fd_done_kernel (pinned);
                                                     [FD_NSLOT]: the synchronous calls' (stream_wait);
                                                     [FD_NSLOT+1]: records gathered, cumulative (fd_gather_kernel) */
  unsigned long sync_token;
  unsigned long * d_flag;
  unsigned long lat_hist[ FDGPU_LAT_BUCKETS ];    /* launch -> verdicts seen by poll, quarter-octave buckets */
  std::deque<int> inflight;      /* slot order */
  struct fdgpu_launcher * launcher;               /* NULL: the caller's thread makes the batch's runtime calls;
                                                     else its launch thread does (fdgpu_ed25519_set_launcher) */
  char lerr[ 192 ];                               /* the launch thread's error, when it faulted the context */
};

/* Context memory: every device buffer of a context and of its slots comes from ctx_dev_alloc and every pinned
   one from ctx_pin_alloc (which also gives its device view, if asked).  Both record the pointer, and
   fdgpu_ed25519_ctx_delete frees from those records: a new buffer is named once, where it is allocated.
   ctx_dev_free gives one back before that (a prepare call that grows its buffers) and takes its record out.
   (d_khash lives inside verify_long only and is not recorded.) */
template< class T > static hipError_t
ctx_dev_alloc( fdgpu_ed25519_ctx_t * ctx, T ** p, size_t sz ) {
  hipError_t e = hipMalloc( (void **)p, sz );
  if( e == hipSuccess ) ctx->dev_mem.push_back( (void *)*p );
  return e;
}
template< class T > static void
ctx_dev_free( fdgpu_ed25519_ctx_t * ctx, T ** p ) {
  if( !*p ) return;
  for( size_t i=0; i<ctx->dev_mem.size(); i++ )
    if( ctx->dev_mem[i] == (void *)*p ) { ctx->dev_mem.erase( ctx->dev_mem.begin() + (long)i ); break; }
  (void)hipFree( *p );
  *p = NULL;
}
template< class T, class U = T > static hipError_t
ctx_pin_alloc( fdgpu_ed25519_ctx_t * ctx, T ** p, size_t sz, U ** dev = NULL ) {
  hipError_t e = hipHostMalloc( (void **)p, sz, hipHostMallocDefault );
  if( e != hipSuccess ) return e;
  ctx->pin_mem.push_back( (void *)*p );
  return dev ? hipHostGetDevicePointer( (void **)dev, (void *)*p, 0 ) : hipSuccess;
}

/* Wait for everything queued on st in a synchronous host call.  A blocking
   hipStreamSynchronize sleeps and now and then wakes late (the host-staged
   8192-txn batch: p99 2x its p50); instead fd_done_kernel stores a fresh
   token into a pinned word behind the batch and the host spins on it.  A
   batch that failed never stores it: after FD_SYNC_SPIN_NS the call falls
   back to hipStreamSynchronize, which waits or reports the error.  Only
   for work whose results land in pinned memory: a copy into pageable host
   memory may finish on the host after the stream (pageable = 1 waits the
   HIP way). */
#define FD_SYNC_SPIN_NS 20000000UL
static int stream_wait( fdgpu_ed25519_ctx_t * ctx, hipStream_t st, int pageable ) {
  if( !pageable ) {
    unsigned long tok = ++ctx->sync_token;
    hipLaunchKernelGGL( fd_done_kernel, dim3(1), dim3(1), 0, st, ctx->d_flag + FD_NSLOT, tok, (unsigned long *)NULL );
    if( hipGetLastError() == hipSuccess ) {
      unsigned long t0 = fd_now_ns();
      while( fd_now_ns() - t0 < FD_SYNC_SPIN_NS ) {
        if( ctx->h_flag[ FD_NSLOT ] == tok ) {
          /* the results the caller reads next were stored before the token (fd_done_kernel's release):
             keep those plain loads behind this volatile one */
          std::atomic_thread_fence( std::memory_order_acquire );
          return 0;
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
      }
    }
  }
  hipError_t e = hipStreamSynchronize( st );
  if( e != hipSuccess ) { set_err( "hipStreamSynchronize", e ); return -2; }
  return 0;
}

extern "C" unsigned long
fdgpu_ed25519_set_small_batch_max( fdgpu_ed25519_ctx_t * ctx, unsigned long small_max ) {
  if( !ctx ) return 0UL;
  unsigned long old = ctx->small_max;
  ctx->small_max = small_max;
  return old;
}

/* Latency-path workgroups alone on their CU: each reserves more than half of the CU's 160 KiB LDS (it uses none
   of the extra), so no second such workgroup -- of this batch or of another context's concurrent one -- shares
   its SIMDs.  A small batch runs under one wave per SIMD, its time the per-wave chain; a second wave on the
   SIMD stretches that chain (profiles/r04/n: prep 108 us alone, 206 us beside the other context's walk). */
/* The reservation is derived from the device's LDS per CU (160 KiB on gfx950): mode 1 takes more than half
   of it (84 KiB there), mode 2 more than a third (56 KiB: two fit, three do not).  The kernels' maximum
   dynamic LDS (a process-wide function attribute) is raised once to what mode 1 needs, so contexts with
   different modes never undo each other's; each context keeps its own choice in excl_lds. */
static std::mutex g_excl_mu;
static unsigned   g_excl_max[ 8 ];     /* per kernel: the dynamic LDS its attribute allows (0: not raised yet) */
extern "C" int
fdgpu_ed25519_set_cu_exclusive( fdgpu_ed25519_ctx_t * ctx, int on ) {
  if( !ctx || on < 0 || on > 4 ) return -1;
  /* on (A/B): 1 prep and walk alone on their CU; 2 at most two per CU; 3 the walk alone; 4 the prep alone */
  void const * f[ 8 ] = { (void const *)fd_prep_kernel<0,1>, (void const *)fd_prep_kernel<0,0>, (void const *)fd_dsm8_kernel<0>,
                          (void const *)fd_dsm4_kernel<0,1>, (void const *)fd_dsm4_kernel<0,0>,
                          (void const *)fd_dsm2_kernel<0,1>, (void const *)fd_dsm2_kernel<0,0>,
                          (void const *)fd_prep_kernel<0,1,1> };
  unsigned v[ 8 ] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
  if( on ) {
    HIPCHK( hipSetDevice( ctx->device ), -2 );
    int lds = 0;
    HIPCHK( hipDeviceGetAttribute( &lds, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, ctx->device ), -2 );
    if( lds < 3 * 1024 ) { fd_err = "fdgpu_ed25519_set_cu_exclusive: no LDS size"; return -1; }
    unsigned half = ( (unsigned)lds / 2u + 4096u ) & ~1023u;          /* > 1/2: one workgroup per CU */
    unsigned third = ( (unsigned)lds / 3u + 2048u ) & ~1023u;         /* > 1/3, <= 1/2: two per CU */
    unsigned want = on == 2 ? third : half;
    std::lock_guard<std::mutex> lk( g_excl_mu );
    for( int i=0; i<8; i++ ) {
      hipFuncAttributes a;
      HIPCHK( hipFuncGetAttributes( &a, f[i] ), -2 );
      unsigned st = (unsigned)a.sharedSizeBytes;
      int walk = i >= 2 && i <= 6;
      if( ( on == 3 && !walk ) || ( on == 4 && walk ) ) continue;
      v[i] = st < want ? want - st : 0u;
      unsigned top = st < half ? half - st : 0u;                        /* the most any mode asks of this kernel */
      if( v[i] && g_excl_max[i] < top ) {
        HIPCHK( hipFuncSetAttribute( f[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)top ), -2 );
        g_excl_max[i] = top;
      }
    }
  }
  for( int i=0; i<8; i++ ) ctx->excl_lds[i] = v[i];
  ctx->excl_mode = on;
  return 0;
}

extern "C" int
fdgpu_ed25519_get_cu_exclusive( fdgpu_ed25519_ctx_t const * ctx ) { return ctx ? ctx->excl_mode : 0; }

extern "C" int
fdgpu_ed25519_set_lat_share( fdgpu_ed25519_ctx_t * ctx, unsigned parts ) {
  if( !ctx ) return -1;
  if( !parts ) { ctx->lat_cus = 0UL; return 0; }
  int ncu = 0;
  HIPCHK( hipSetDevice( ctx->device ), -2 );
  HIPCHK( hipDeviceGetAttribute( &ncu, hipDeviceAttributeMultiprocessorCount, ctx->device ), -2 );
  unsigned long free_cus = (unsigned long)ncu > ctx->gather_cus ? (unsigned long)ncu - ctx->gather_cus : 1UL;
  ctx->lat_cus = free_cus / parts ? free_cus / parts : 1UL;
  return 0;
}

extern "C" char const * fdgpu_last_error( void ) { return fd_err.c_str(); }

/* the synchronous host calls stage through slot 0: only when the async
   pipeline holds nothing */
static int async_busy( fdgpu_ed25519_ctx_t const * ctx ) {
  if( !ctx->inflight.empty() ) return 1;
  for( int i=0; i<FD_NSLOT; i++ ) if( ctx->slot[i].txn_cnt ) return 1;
  return 0;
}

/* the engine path a batch of nsig signatures takes: latency-path lanes per signature in the walk (8, 4, 2,
   1) or FDGPU_PATH_THROUGHPUT(_FULL) -- launch_batch's choice, also known before its launch (slot_launch_) */
static int pick_path( fdgpu_ed25519_ctx_t const * ctx, unsigned long nsig ) {
  if( !nsig ) return FDGPU_PATH_NONE;
  if( nsig <= ctx->small_max ) {
    /* lanes per signature in the DSM: 4 while a quad per signature still fits one wave per
       SIMD (n <= 16K), 2 while a pair does (n <= 32K), else 1 (configs[0]'s 64K: 0.88 ms
       against 0.92 on the throughput path and 1.08 with two lanes, tools/configs0_ab.py) */
    int lanes = ctx->dsm_lanes ? ctx->dsm_lanes : ( nsig <= FD_DSM8_MAX && ctx->half ? 8 : nsig <= FD_DSM4_MAX ? 4 :
                                                    nsig <= FD_DSM2_MAX ? 2 : 1 );
    if( lanes == 8 && !ctx->half ) lanes = 4;        /* the term split needs the half-size walk */
    /* an exclusive walk (one workgroup of 256 lanes per CU, two in mode 2) within the context's CU budget:
       fewer lanes per signature, fewer workgroups (fdgpu_ed25519_set_lat_share) */
    int excl_walk = ctx->excl_mode == 1 || ctx->excl_mode == 2 || ctx->excl_mode == 3;
    if( !ctx->dsm_lanes && ctx->lat_cus && excl_walk ) {
      unsigned long budget = ctx->lat_cus * ( ctx->excl_mode == 2 ? 2UL : 1UL );
      unsigned long wg = ( nsig + FD_WG - 1UL ) / FD_WG;                 /* workgroups per lane of a signature */
      while( lanes > 1 && (unsigned long)lanes * wg > budget ) lanes >>= 1;
    }
    return lanes;
  }
  return ctx->half ? FDGPU_PATH_THROUGHPUT : FDGPU_PATH_THROUGHPUT_FULL;
}

/* The words after d_slow[max_sig]: a batch's device-side counts (slow_word) */
enum {
  FD_SW_SLOW     = 0,   /* the slow list's count */
  FD_SW_KEYS     = 1,   /* the distinct keys' count; from here ucnt[0..2] of fd_keydedup_kernel and fd_decode_kernel */
  FD_SW_DISTINCT = 2,   /* were most keys of the batch before distinct? */
  FD_SW_SAMPLE   = 3,   /* the count of the sample that decides it */
  FD_SW_HOT      = 4,   /* the hot keys, then the hot and the cold signatures, the fixed-base keys claimed and the
                           fixed-base signatures: the counters of fd_keysplit_kernel and fd_keyclass_kernel (FD_KC_*) */
  FD_SW_FBSLOW   = 9,   /* the count of the fixed-base R check's list (d_fslow) */
  FD_SW_KCACHE   = 10,  /* the key cache's hits, misses and builds, the hand's start and the hand (FD_KC_HIT.., counted from
                           FD_SW_HOT); the hand alone outlives a batch */
  FD_SW_CNT      = 24 };                /* (... and the full slots' tickets, keys and signatures, DESIGN 18: FD_KC_PTIX..,
                                           the pinned keys' and the wide tables' counts, DESIGN 19, 20: ..FD_KC_FWS) */
static u32 * slow_word( fdgpu_ed25519_ctx_t const * ctx, int w ) { return ctx->d_slow + ctx->max_sig + w; }

/* What every kernel launch of one batch shares */
struct fd_batch {
  unsigned char const *    d_payload;
  fdgpu_txn_desc_t const * d_desc;
  u32                      nsig;
  unsigned                 sg;     /* workgroups of one lane per signature */
  i8 *                     code;   /* the per-signature codes */
  hipStream_t              st;
  hipEvent_t *             ev;     /* recorded while ctx->timing: [0] prep start, [1] walk start, [2] walk end,
                                      [3] reduce end, [4] (half-size throughput path) the decode kernel's end */
};

/* Latency path: a batch that cannot fill the GPU, so its time is the sum of the kernels' per-wave instruction
   streams -- decode A, decode R and hash side by side in one launch (fd_prep_kernel), then the walk on `lanes`
   lanes per signature with R compared at its end (no R-check chain and its inversion). */
static int launch_latency( fdgpu_ed25519_ctx_t * ctx, fd_batch const & b, int lanes ) {
  u32 nsig = b.nsig; unsigned sg = b.sg; i8 * code = b.code; hipStream_t st = b.st;
  int hs = ctx->half;                                           /* half-size scalars */
  int qs = hs && ctx->quad_sha >= 0 && nsig <= FD_QSHA_MAX;     /* the hash role on quads (fd_sha512_RAM_quad) */
  int d2 = lanes > 1;
  u32 * slow_cnt = slow_word( ctx, FD_SW_SLOW );
  /* half-size: the A and R lanes build both tables, the hash lane (c0, c1, s'); else the A lane builds -A's
     table for the 4- and 2-lane walks, and fd_table_kernel builds it for the one-lane walk */
  hipLaunchKernelGGL( ( qs ? fd_prep_kernel<0,1,1> : hs ? fd_prep_kernel<0,1> : fd_prep_kernel<0,0> ),
                      dim3( ( qs ? 6 : 3 )*sg ), dim3(FD_WG), ctx->excl_lds[ qs ? 7 : hs ? 0 : 1 ], st, b.d_payload, b.d_desc,
                      ctx->d_map, nsig, (u32)sg, ctx->semantics, ctx->d_pstat, ctx->d_Rxy, ctx->d_Axy, code, ctx->d_digA,
                      ctx->d_digB, hs || d2 ? ctx->d_tab : (uint4 *)NULL, (uint4 const *)ctx->d_khash,
                      hs ? ctx->d_tabR : (uint4 *)NULL, hs ? ctx->d_digR : (i8 *)NULL, hs ? ctx->d_slow : (u32 *)NULL,
                      hs ? slow_cnt : (u32 *)NULL, hs ? ctx->half_force_slow : 0u, hs ? ctx->d_htop : (unsigned char *)NULL );
  if( !hs && !d2 )
    hipLaunchKernelGGL( fd_table_kernel, dim3(sg), dim3(FD_WG), 0, st, nsig, ctx->semantics, ctx->d_pstat, code,
                        ctx->d_Axy, ctx->d_tab );
  if( ctx->timing ) hipEventRecord( b.ev[1], st );
  if( lanes==8 )
    hipLaunchKernelGGL( fd_dsm8_kernel<0>, dim3(8*sg), dim3(FD_WG), ctx->excl_lds[2], st, nsig, ctx->d_tab, ctx->d_tabR,
                        ctx->d_digA, ctx->d_digR, ctx->d_digB, ctx->d_btab, ctx->d_btab2, code, ctx->semantics, ctx->d_pstat,
                        ctx->d_htop, ctx->d_Rxy, ctx->d_slow, slow_cnt );
  else if( lanes==4 || lanes==2 )
    hipLaunchKernelGGL( ( lanes==4 ? ( hs ? fd_dsm4_kernel<0,1> : fd_dsm4_kernel<0,0> )
                                   : ( hs ? fd_dsm2_kernel<0,1> : fd_dsm2_kernel<0,0> ) ),
                        dim3(lanes*sg), dim3(FD_WG), ctx->excl_lds[ ( lanes==4 ? 3 : 5 ) + !hs ], st, nsig, ctx->d_tab,
                        ctx->d_Rxy, ctx->d_digA, ctx->d_digB, ctx->d_btab, code, ctx->semantics, ctx->d_pstat,
                        ctx->d_tabR, ctx->d_digR, ctx->d_btab2, ctx->d_htop, ctx->d_slow, slow_cnt );
  else if( hs )                                /* one lane: the half-size walk, result codes at its start */
    hipLaunchKernelGGL( fd_dsmh_kernel<0>, dim3(sg), dim3(FD_WG), 0, st, nsig, ctx->d_tab, ctx->d_tabR, ctx->d_digA,
                        ctx->d_digR, ctx->d_digB, ctx->d_btab, ctx->d_btab2, code, ctx->d_Rxy, ctx->d_slow, slow_cnt, 0u,
                        ctx->d_pstat, ctx->d_htop, 1, ctx->semantics, (u32 const *)NULL, (u32 const *)NULL,
                        (u32 const *)NULL, (u32 const *)NULL, (uint4 const *)NULL, (uint4 const *)NULL,
                        (u32 const *)NULL, (uint4 const *)NULL, (uint4 const *)NULL, (u32 *)NULL, (u32 const *)NULL,
                        (u32 *)NULL, (uint4 const *)NULL, 0u );
  else                                         /* one lane, full length (no carry fold up to nofold_max) */
    hipLaunchKernelGGL( ( nsig <= ctx->nofold_max ? fd_dsm_kernel<0> : fd_dsm_kernel<1> ), dim3(sg), dim3(FD_WG), 0, st,
                        nsig, ctx->d_tab, ctx->d_Rxy, ctx->d_digA, ctx->d_digB, ctx->d_btab, code, ctx->d_P, 0 );
  if( ctx->timing ) hipEventRecord( b.ev[2], st );
  if( hs && lanes <= 1 )                       /* slow list (normally empty); the 8/4/2-lane walks ran it */
    hipLaunchKernelGGL( fd_dsm_slowl_kernel<0>, dim3(sg), dim3(FD_WG), 0, st, nsig, ctx->d_tab, ctx->d_Rxy, ctx->d_digA,
                        ctx->d_digB, ctx->d_btab, code, ctx->d_slow, slow_cnt, ctx->semantics, ctx->d_pstat );
  return 0;
}

/* Half-size throughput path: each distinct key decoded once (fd_keydedup_kernel), the signatures of repeated keys
   ordered ahead of the others (fd_keysplit_kernel), fd_decode_kernel (A and R with their tables), fd_hashh_kernel
   (result codes, hash, (c0, c1, s'), the hot keys' high tables), then the walk fd_dsmh_kernel with the head of the
   slow list in its first blocks, and fd_dsm_slow_kernel for the rest.  With fixed-base keys (kf) also
   fd_keyclass_kernel and fd_keyclaim_kernel ahead of the split, fd_ftab_kernel ahead of the walk and the R-check
   chain behind it; the tables stay in the context's key cache, so a batch builds only the keys it
   did not find there. */
static int launch_half( fdgpu_ed25519_ctx_t * ctx, fd_batch const & b ) {
  u32 nsig = b.nsig; unsigned sg = b.sg; i8 * code = b.code; hipStream_t st = b.st;
  int kd = ctx->key_dedup, ks = ctx->key_split, kf = ctx->key_fixed;   /* (ks needs kd, kf needs ks) */
  u32 * slow_cnt = slow_word( ctx, FD_SW_SLOW ), * ucnt = slow_word( ctx, FD_SW_KEYS );
  /* kd: A's status and -A's table are the representative's.  ks: lane i <-> signature order[i], hot blocks then
     cold blocks (at most sg + 1 of them) */
  u32 const * arep = kd ? ctx->d_arep : NULL, * order = ks ? ctx->d_order : NULL, * hidx = ks ? ctx->d_hidx : NULL;
  u32 const * kscnt = ks ? slow_word( ctx, FD_SW_HOT ) : NULL;
  /* kf: the worst case of keys that can be fixed-base in this batch, min( nsig / fb_min, fb_cap ): it sizes the grids
     of fd_keyclaim_kernel, of fbase_build's blocks and of fd_ftab_kernel */
  unsigned long fkeys = kf ? nsig / ctx->fb_min : 0UL; if( fkeys > ctx->fb_cap ) fkeys = ctx->fb_cap;
  fd_kcache kc = {}; unsigned iblk = 0u;
  /* pinned keys: fd_keyclass_kernel gives every representative a class, so the kernels that read fidx[] only
     where the key's count reached the bound read it everywhere (their bound is 0), and the R-check chain behind the
     walk runs whatever nsig is: a batch of one signature can be fixed-base.  Without pins (npin = 0) every
     argument and every launch is as before */
  u32 npin = kf ? ctx->npin : 0u, fbm = npin ? 0u : ctx->fb_min;
  if( kd ) {
    /* the table cleared for this batch -- the smallest power of two of slots that is twice its signatures, so a
       small batch on a large context clears little -- then (ks) the signatures per key counted and the batch
       partitioned into hot and cold */
    u32 slots = 64u;
    if( !ctx->kd_tiny ) while( slots < ctx->kd_slots && slots < 2u*nsig ) slots <<= 1;
    /* kf: the key cache's index of this batch in front of the table, cleared with it.  With the cache off, or after a
       launch that failed (a slot claimed but never built), every slot is emptied first: every key then misses and
       builds, with the same kernels and launches */
    if( kf ) {
      kc.key = ctx->d_skey; kc.state = ctx->d_sstate; kc.birth = ctx->d_sbirth; kc.stat = ctx->d_sstat; kc.idx = ctx->d_kidx;
      kc.imask = ctx->kc_iwords - 1u; kc.iprobes = ctx->kc_iprobes; kc.fcap = ctx->fb_cap;
      if( !++ctx->kc_batch ) { ctx->kc_batch = 1u; ctx->kc_dirty = 1; }        /* (the number wrapped: old stamps mean nothing) */
      kc.batch = ctx->kc_batch;
      kc.full = ctx->d_sfull; kc.plist = ctx->d_plist; kc.pmax = ctx->pmax; kc.fnow = ctx->kfull_mode == 2;
      kc.npin = ctx->npin;
      int clear = ctx->kc_mode == 1 || ctx->kc_dirty;
      ctx->kc_dirty = 2;                                   /* (until launch_batch has launched all of this batch) */
      if( clear ) HIPCHK( hipMemsetAsync( ctx->d_sstate, 0, ( ctx->fb_cap ? ctx->fb_cap : 1UL ) * 3 * sizeof(u32), st ), -3 );   /* (state, birth, full) */
      iblk = ( ctx->fb_cap + FD_WG - 1u ) / FD_WG;
    }
    HIPCHK( hipMemsetAsync( kf ? ctx->d_kidx : ctx->d_ktab, 0, ( (size_t)slots + ( kf ? ctx->kc_iwords : 0u ) ) * sizeof(u32), st ), -3 );
    if( ks ) HIPCHK( hipMemsetAsync( ctx->d_kcnt, 0, (size_t)nsig * sizeof(u32), st ), -3 );
    u32 seed = ++ctx->kd_seed;
    hipLaunchKernelGGL( ( ks ? fd_keydedup_kernel<1> : fd_keydedup_kernel<0> ), dim3(iblk + sg), dim3(FD_WG), 0, st, b.d_payload,
                        b.d_desc, ctx->d_map, nsig, ctx->d_ktab, slots - 1u, seed, ctx->kd_probes, ctx->d_arep,
                        ctx->d_ulist, ucnt, ctx->d_pstat, FD_KD_SBLK( sg ), ks ? ctx->d_kcnt : (u32 *)NULL,
                        kf && ctx->fb_min > ctx->hot_min ? ctx->fb_min : ks ? ctx->hot_min : 0u, (u32)iblk, kc );
    if( kf ) {
      hipLaunchKernelGGL( fd_keyclass_kernel, dim3(sg), dim3(FD_WG), 0, st, (u32 const *)ctx->d_ulist, (u32 const *)ucnt,
                          (u32 const *)ctx->d_kcnt, ctx->fb_min, ctx->d_fidx, ctx->d_mlist, slow_word( ctx, FD_SW_HOT ),
                          b.d_payload, b.d_desc, (u32 const *)ctx->d_map, seed, ctx->d_astat, kc );
      if( fkeys ) {
        /* (... and, in the blocks after, the P_j of the slots fd_keyclass_kernel promoted: 24 lanes a slot, the
           worst case of pmax slots, blocks beyond the device-side count return at once) */
        unsigned cblk = (unsigned)( ( fkeys + FD_WG - 1UL ) / FD_WG ), pbk = (unsigned)( ( 24UL * ctx->pmax + FD_WG - 1 ) / FD_WG );
        /* (... and behind those the 16 extra base points of the promoted slots below wcap) */
        unsigned wbk = ctx->wcap ? (unsigned)( ( 16UL * ctx->pmax + FD_WG - 1 ) / FD_WG ) : 0u;
        hipLaunchKernelGGL( fd_keyclaim_kernel, dim3( cblk + pbk + wbk ), dim3(FD_WG), 0, st,
                            (u32 const *)ctx->d_mlist, slow_word( ctx, FD_SW_HOT ), ctx->d_fidx, ctx->d_flist, b.d_payload,
                            b.d_desc, (u32 const *)ctx->d_map, kc, (u32)cblk, ctx->d_fbase, (u32)pbk, ctx->d_wbase, ctx->wcap );
      }
    }
    if( ks )
      hipLaunchKernelGGL( fd_keysplit_kernel, dim3(sg), dim3(FD_WG), 0, st, nsig, (u32 const *)ctx->d_arep,
                          (u32 const *)ctx->d_kcnt, ctx->hot_min, ctx->d_hidx, ctx->d_hlist, ctx->d_order,
                          slow_word( ctx, FD_SW_HOT ), ctx->hot_cap, (u32 const *)( kf ? ctx->d_fidx : NULL ),
                          kf ? ctx->d_orderh : (u32 *)NULL, kf ? fbm : 0u, npin );
  }
  /* kd: A lanes over the representatives in the first sg blocks, R lanes over every signature; else lanes 2s, 2s+1 */
  /* kf: the R lanes by place in the partition (sg + 2 blocks at most), none for the fixed-base signatures */
  hipLaunchKernelGGL( fd_decode_kernel, dim3( kf ? 2*sg + 2 : kd ? 2*sg : (unsigned)( ( 2UL*nsig + FD_WG - 1 ) / FD_WG ) ),
                      dim3(FD_WG), 0, st,
                      b.d_payload, b.d_desc, ctx->d_map, nsig, 1, ctx->d_pstat, ctx->d_Rxy, ctx->d_Axy, ctx->d_tab, ctx->d_tabR,
                      kd ? (u32 const *)ctx->d_ulist : NULL, kd ? ucnt : (u32 *)NULL,
                      kd ? ctx->d_astat : (unsigned char *)NULL, kd ? (u32)sg : 0u, kf ? order : (u32 const *)NULL,
                      (u32 const *)( kf ? ctx->d_orderh : NULL ), kf ? kscnt : (u32 const *)NULL,
                      (u32 const *)( kf ? ctx->d_kcnt : NULL ), kf ? fbm : 0u, (u32 const *)( kf ? ctx->d_fidx : NULL ),
                      (u32 const *)( kf ? ctx->d_sbirth : NULL ), kc.batch, (u32 const *)( kf ? ctx->d_sfull : NULL ),
                      kf ? ctx->wcap : 0u );
  if( ctx->timing ) hipEventRecord( b.ev[4], st );     /* (the decode kernel's own time, fdgpu_ed25519_kernel_ms 3) */
  /* ks: the high tables of the hot keys in the first hb blocks (two lanes per key, the worst case of nsig / hot_min
     keys; blocks beyond the device-side count return at once), then the hot and the cold blocks */
  unsigned hb = ks ? (unsigned)( ( 2UL * ( nsig / ctx->hot_min ) + FD_WG - 1 ) / FD_WG ) : 0u;
  /* kf: likewise the fixed-base keys' [2^(32t)](-A) in the next fbk blocks (lpk = eight lanes per key, the worst case of
     min( nsig / fb_min, fb_cap ) keys); their entries after the hash (fd_ftab_kernel: two keys per block).  Both run
     over the keys that claimed a slot in this batch: none, when every key was resident */
  /* with key_full = 2 a claim builds all 32 P_j (32 lanes per key) and all four groups of tables; the slots
     promoted in this batch (at most pmax, the count on the device) build three groups each in fd_ftab_kernel */
  unsigned lpk = kf && ctx->kfull_mode == 2 ? 32u : 8u, cg = lpk / 8u;
  unsigned long pkeys = fkeys ? ctx->pmax : 0UL;
  unsigned fbk = (unsigned)( ( lpk * fkeys + FD_WG - 1 ) / FD_WG );
  hipLaunchKernelGGL( ( ks ? fd_hashh_kernel<1> : fd_hashh_kernel<0> ), dim3( ks ? hb + fbk + sg + ( kf ? 2 : 1 ) : sg ),
                      dim3(FD_WG), 0, st,
                      b.d_payload, b.d_desc, ctx->d_map, nsig, ctx->semantics, ctx->d_pstat, code, ctx->d_digA, ctx->d_digR,
                      ctx->d_digB, ctx->d_slow, slow_cnt, (uint4 const *)ctx->d_khash, ctx->half_force_slow, ctx->d_htop,
                      arep, (unsigned char const *)( kd ? ctx->d_astat : NULL ), ks ? ctx->d_order : (u32 *)NULL, kscnt,
                      (u32 const *)( ks ? ctx->d_hlist : NULL ), (uint4 const *)( ks ? ctx->d_Axy : NULL ),
                      ks ? ctx->d_htab : (uint4 *)NULL, (u32)hb, (u32 const *)( kf ? ctx->d_orderh : NULL ),
                      (u32 const *)( kf ? ctx->d_flist : NULL ), kf ? ctx->d_fbase : (uint4 *)NULL, (u32)fbk,
                      kf ? ctx->d_sstat : (unsigned char *)NULL, kf ? ctx->d_Rxy : (uint4 *)NULL, (u32)lpk );
  if( fkeys ) {
    /* the wide tables of the slots below wcap, 24 items a slot: of the promoted slots, and of the claims'
       when a claim fills its slot at once (their 16 extra base points first, from the P_4t the hash launch stored).
       The grid holds the worst case of both lists; wcap = 0: the parent's launches */
    unsigned wnow = ctx->wcap && ctx->kfull_mode == 2;
    unsigned long witems = ctx->wcap ? 24UL * ( ( wnow ? fkeys : 0UL ) + pkeys ) : 0UL;
    if( wnow )
      hipLaunchKernelGGL( fd_wbase_kernel, dim3( (unsigned)( ( 16UL * fkeys + FD_WG - 1 ) / FD_WG ) ), dim3(FD_WG), 0, st, kscnt,
                          (u32 const *)ctx->d_flist, (unsigned char const *)ctx->d_astat, (uint4 const *)ctx->d_fbase,
                          ctx->d_wbase, ctx->wcap );
    hipLaunchKernelGGL( fd_ftab_kernel, dim3( (unsigned)( ( cg * fkeys + 3UL * pkeys + witems + 1UL ) / 2UL ) ), dim3(FD_WG), 0, st, kscnt,
                        (u32 const *)ctx->d_flist, (unsigned char const *)ctx->d_astat, (uint4 const *)ctx->d_fbase,
                        ctx->d_ftab, (u32)cg, (u32 const *)ctx->d_plist, ctx->pmax, (uint4 const *)ctx->d_wbase, ctx->d_wtab,
                        ctx->wcap, (u32)wnow );
  }
  if( ctx->timing ) hipEventRecord( b.ev[1], st );
  /* slow list: its head in fd_dsmh_kernel's first nsb blocks (room for 1/64 of the batch), the rest (if any) in
     fd_dsm_slow_kernel */
  unsigned nsb = ( sg + 63u ) / 64u;
  int fold = nsig > ctx->nofold_max;
  hipLaunchKernelGGL( ( fold ? ( ks ? fd_dsmh_kernel<1,1> : fd_dsmh_kernel<1,0> )
                             : ( ks ? fd_dsmh_kernel<0,1> : fd_dsmh_kernel<0,0> ) ),
                      dim3( nsb + sg + ( kf ? 2u : ks ? 1u : 0u ) ), dim3(FD_WG), 0, st, nsig, ctx->d_tab, ctx->d_tabR, ctx->d_digA,
                      ctx->d_digR, ctx->d_digB, ctx->d_btab, ctx->d_btab2, code, ctx->d_Rxy, ctx->d_slow, slow_cnt, nsb,
                      ctx->d_pstat, ctx->d_htop, 0, ctx->semantics, arep, order, kscnt, hidx,
                      (uint4 const *)( ks ? ctx->d_htab : NULL ), (uint4 const *)( ks ? ctx->d_btabh : NULL ),
                      (u32 const *)( kf ? ctx->d_fidx : NULL ), (uint4 const *)( kf ? ctx->d_ftab : NULL ),
                      (uint4 const *)( kf ? ctx->d_btabf : NULL ), kf ? ctx->d_P : (u32 *)NULL,
                      (u32 const *)( kf ? ctx->d_sfull : NULL ), kf ? slow_word( ctx, FD_SW_HOT ) + FD_KC_FFS : (u32 *)NULL,
                      (uint4 const *)( kf ? ctx->d_wtab : NULL ), kf ? ctx->wcap : 0u );
  if( ctx->timing ) hipEventRecord( b.ev[2], st );
  if( fkeys || npin ) {
    /* the fixed-base signatures' R, compared undecoded: the full-length path's chain over the fixed-base segment of
       order[] (the worst case of blocks; those beyond the device-side count return at once), with a list and a
       counter of its own -- fd_dsm_slow_kernel below still reads the half-size slow list's */
    u32 const * fcnt = kscnt + FD_KC_FB; u32 * fslow_cnt = slow_word( ctx, FD_SW_FBSLOW );
    hipLaunchKernelGGL( fd_rprod_kernel, dim3(sg), dim3(FD_WG), 0, st, nsig, code, ctx->d_P, ctx->d_O, ctx->d_blk, fslow_cnt,
                        order, fcnt );
    hipLaunchKernelGGL( fd_rinv_kernel, dim3((sg + FD_WG - 1)/FD_WG), dim3(FD_WG), 0, st, sg, ctx->d_blk, fcnt );
    hipLaunchKernelGGL( fd_rcheck_kernel, dim3(sg), dim3(FD_WG), 0, st, nsig, code, ctx->d_Rxy, ctx->d_P, ctx->d_O, ctx->d_blk,
                        ctx->d_fslow, fslow_cnt, order, fcnt, 4u, FD_PEND_FBREQ );
    hipLaunchKernelGGL( fd_rslow_kernel, dim3(sg), dim3(FD_WG), 0, st, nsig, ctx->semantics, code, ctx->d_Rxy, ctx->d_P,
                        ctx->d_fslow, fslow_cnt, order, 4u );
  }
  hipLaunchKernelGGL( ( fold ? fd_dsm_slow_kernel<1> : fd_dsm_slow_kernel<0> ), dim3(sg), dim3(FD_WG), 0, st, nsig,
                      ctx->d_tab, ctx->d_Rxy, ctx->d_digA, ctx->d_digB, ctx->d_btab, code, ctx->d_slow, slow_cnt,
                      nsb * FD_WG, arep, order );
  return 0;
}

/* Full-length throughput path (half = 0): fd_decode_kernel (A only), fd_hash_kernel, fd_table_kernel, the walk
   fd_dsm_kernel, which leaves P for the deferred R check: fd_rprod_kernel, fd_rinv_kernel, fd_rcheck_kernel and
   fd_rslow_kernel. */
static int launch_full( fdgpu_ed25519_ctx_t * ctx, fd_batch const & b ) {
  u32 nsig = b.nsig; unsigned sg = b.sg; i8 * code = b.code; hipStream_t st = b.st;
  u32 * slow_cnt = slow_word( ctx, FD_SW_SLOW );
  hipLaunchKernelGGL( fd_decode_kernel, dim3(sg), dim3(FD_WG), 0, st, b.d_payload, b.d_desc, ctx->d_map, nsig, 0,
                      ctx->d_pstat, ctx->d_Rxy, ctx->d_Axy, (uint4 *)NULL, (uint4 *)NULL, (u32 const *)NULL,
                      (u32 *)NULL, (unsigned char *)NULL, 0u, (u32 const *)NULL, (u32 const *)NULL, (u32 const *)NULL,
                      (u32 const *)NULL, 0u, (u32 const *)NULL, (u32 const *)NULL, 0u, (u32 const *)NULL, 0u );
  hipLaunchKernelGGL( fd_hash_kernel, dim3(sg), dim3(FD_WG), 0, st, b.d_payload, b.d_desc, ctx->d_map, nsig,
                      ctx->semantics, 1, ctx->d_pstat, code, ctx->d_digA, ctx->d_digB, ctx->d_Rxy,
                      (uint4 const *)ctx->d_khash );
  hipLaunchKernelGGL( fd_table_kernel, dim3(sg), dim3(FD_WG), 0, st, nsig, ctx->semantics,
                      (unsigned char const *)NULL, code, ctx->d_Axy, ctx->d_tab );
  if( ctx->timing ) hipEventRecord( b.ev[1], st );
  /* no carry fold up to nofold_max (<= 2 waves per SIMD: latency-bound, independent column chains) */
  hipLaunchKernelGGL( ( nsig <= ctx->nofold_max ? fd_dsm_kernel<0> : fd_dsm_kernel<1> ), dim3(sg), dim3(FD_WG), 0, st,
                      nsig, ctx->d_tab, ctx->d_Rxy, ctx->d_digA, ctx->d_digB, ctx->d_btab, code, ctx->d_P, 1 );
  if( ctx->timing ) hipEventRecord( b.ev[2], st );
  hipLaunchKernelGGL( fd_rprod_kernel, dim3(sg), dim3(FD_WG), 0, st, nsig, code, ctx->d_P, ctx->d_O, ctx->d_blk, slow_cnt,
                      (u32 const *)NULL, (u32 const *)NULL );
  hipLaunchKernelGGL( fd_rinv_kernel, dim3((sg + FD_WG - 1)/FD_WG), dim3(FD_WG), 0, st, sg, ctx->d_blk, (u32 const *)NULL );
  hipLaunchKernelGGL( fd_rcheck_kernel, dim3(sg), dim3(FD_WG), 0, st, nsig, code, ctx->d_Rxy, ctx->d_P, ctx->d_O, ctx->d_blk,
                      ctx->d_slow, slow_cnt, (u32 const *)NULL, (u32 const *)NULL, 2u, FD_PEND_REQ );
  hipLaunchKernelGGL( fd_rslow_kernel, dim3(sg), dim3(FD_WG), 0, st, nsig, ctx->semantics, code, ctx->d_Rxy, ctx->d_P,
                      ctx->d_slow, slow_cnt, (u32 const *)NULL, 2u );
  return 0;
}

/* flags: 1 = the map is written already (fused into fd_parse_kernel), 2 = no reduce (fd_finish_kernel does it) */
static int launch_batch( fdgpu_ed25519_ctx_t * ctx, unsigned char const * d_payload, fdgpu_txn_desc_t const * d_desc,
                         unsigned long txn_cnt, unsigned long sig_cnt, i8 * d_txn_out, i8 * d_sig_out, hipStream_t st,
                         unsigned char const * d_pflag = NULL, int flags = 0 ) {
  if( !txn_cnt ) return 0;
  fd_batch b = { d_payload, d_desc, (u32)sig_cnt, (unsigned)( (sig_cnt + FD_WG - 1) / FD_WG ),
                 d_sig_out ? d_sig_out : ctx->d_code, st, ctx->ev };
  if( ctx->timing ) { b.ev = ctx->ring[ ctx->ring_cnt % FD_NRING ]; ctx->ring_cnt++; }
  unsigned tg = (unsigned)( (txn_cnt + FD_WG - 1) / FD_WG );
  ctx->last_path = pick_path( ctx, b.nsig );
  if( b.nsig ) {
    if( !( flags & 1 ) )
      hipLaunchKernelGGL( fd_expand_kernel, dim3(tg), dim3(FD_WG), 0, st, d_desc, (u32)txn_cnt, ctx->d_map, b.nsig,
                          slow_word( ctx, FD_SW_SLOW ) );
    if( ctx->timing ) hipEventRecord( b.ev[0], st );
    int err = b.nsig <= ctx->small_max ? launch_latency( ctx, b, ctx->last_path )
            : ctx->half                ? launch_half( ctx, b ) : launch_full( ctx, b );
    if( err ) return err;
  }
  if( !( flags & 2 ) )
    hipLaunchKernelGGL( fd_reduce_kernel, dim3(tg), dim3(FD_WG), 0, st, d_desc, (u32)txn_cnt, b.nsig, b.code, d_pflag, d_txn_out );
  if( ctx->timing ) hipEventRecord( b.ev[3], st );
  HIPCHK( hipGetLastError(), -3 );
  if( ctx->kc_dirty == 2 ) ctx->kc_dirty = 0;           /* (launch_half: every launch of the batch was taken) */
  return 0;
}

/* Test / A/B options of contexts created from now on (fdgpu_debug_set_opts).
   Process-wide, behind a mutex; the defaults are the product's choices. */
static std::mutex g_dbg_mu;
static fdgpu_debug_opts_t g_dbg = { -1, 0u, -1L, 0, -1L, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
static void debug_opts_get( fdgpu_debug_opts_t * o ) { std::lock_guard<std::mutex> lk( g_dbg_mu ); *o = g_dbg; }

extern "C" void
fdgpu_debug_set_opts( fdgpu_debug_opts_t const * opts ) {
  std::lock_guard<std::mutex> lk( g_dbg_mu );
  if( opts ) g_dbg = *opts;
  else       g_dbg = fdgpu_debug_opts_t{ -1, 0u, -1L, 0, -1L, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
}

/* staging + device buffers of async slot i (once) */
static int
slot_bufs( fdgpu_ed25519_ctx_t * ctx, int i ) {
  fd_slot & sl = ctx->slot[i];
  if( sl.h_payload ) return 0;
  unsigned long mp = ctx->max_payload, mt = ctx->max_txn;
  HIPCHK( hipSetDevice( ctx->device ), -1 );
  HIPCHK( ctx_pin_alloc( ctx, &sl.h_payload, mp + FD_ARENA_SLACK ), -1 );
  HIPCHK( ctx_pin_alloc( ctx, &sl.h_desc, mt * sizeof(fdgpu_txn_desc_t), &sl.hd_desc ), -1 );
  HIPCHK( ctx_pin_alloc( ctx, &sl.h_txn_out, mt, &sl.hd_txn_out ), -1 );
  HIPCHK( ctx_pin_alloc( ctx, &sl.h_tags, mt * sizeof(unsigned long) ), -1 );
  HIPCHK( ctx_dev_alloc( ctx, &sl.d_payload, mp + FD_ARENA_SLACK + FD_IMG_TAIL ), -1 );   /* + the last gathered record's image */
  HIPCHK( ctx_dev_alloc( ctx, &sl.d_desc, mt * sizeof(fdgpu_txn_desc_t) ), -1 );
  HIPCHK( ctx_dev_alloc( ctx, &sl.d_txn_out, mt ), -1 );
  memset( sl.h_payload, 0, FD_ARENA_SLACK );
  return 0;
}

__global__ void fd_clock_kernel( unsigned long * out ) {
  __hip_atomic_store( out, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
}

/* GPU clock -> host clock offset, from the shortest of three probe launches on the context's idle
   stream at creation (error <= half that round trip, ~10 us) */
static void gclk_calibrate( fdgpu_ed25519_ctx_t * ctx ) {
  unsigned long volatile * w = (unsigned long volatile *)( ctx->h_stamp + 2*FD_NSLOT );
  double best = 1e30;
  for( int k=0; k<3; k++ ) {
    w[0] = 0UL;
    unsigned long t0 = fd_now_ns();
    hipLaunchKernelGGL( fd_clock_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->d_stamp + 2*FD_NSLOT );
    if( hipStreamSynchronize( ctx->stream ) != hipSuccess || !w[0] ) return;
    unsigned long t1 = fd_now_ns();
    if( (double)( t1 - t0 ) < best ) { best = (double)( t1 - t0 ); ctx->gclk_off_ns = (double)w[0] * 10.0 - 0.5 * ( (double)t0 + (double)t1 ); }
  }
  ctx->gclk_ok = 1;
}

/* allocations of a new context; on failure the caller deletes the
   partially built context (every handle starts NULL) */
static int
ctx_init( fdgpu_ed25519_ctx_t * ctx, int device, unsigned long max_txn, unsigned long max_sig,
          unsigned long max_payload_bytes, int semantics ) {
  ctx->device = device; ctx->semantics = semantics; ctx->timing = 0;
  ctx->max_txn = max_txn; ctx->max_sig = max_sig; ctx->max_payload = max_payload_bytes;
  size_t ns = max_sig;
  HIPCHK( hipStreamCreateWithFlags( &ctx->stream, hipStreamNonBlocking ), -1 );

  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_map,  ns * sizeof(u32) ), -1 );
  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_code, ns ), -1 );
  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_pstat, 2*ns ), -1 );
  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_tab,  ns * FD_ATAB_STORED * 8 * sizeof(uint4) ), -1 );
  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_Rxy,  ns * 4 * sizeof(uint4) ), -1 );
  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_Axy,  ns * 4 * sizeof(uint4) ), -1 );
  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_digA, ns * 64 ), -1 );
  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_digB, ns * FD_BDIG * sizeof(short) ), -1 );
  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_btab, FD_BTAB_ENTRIES * 6 * sizeof(uint4) ), -1 );
  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_rdesc, max_txn * sizeof(fdgpu_txn_desc_t) ), -1 );
  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_pflag, max_txn ), -1 );
  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_P, ns * 30 * sizeof(u32) ), -1 );
  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_O, ns * 10 * sizeof(u32) ), -1 );
  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_blk, ( ( ns + FD_WG - 1 ) / FD_WG ) * 10 * sizeof(u32) ), -1 );
  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_slow, ( ns + FD_SW_CNT ) * sizeof(u32) ), -1 );   /* the list + the batch's counts (slow_word) */
  HIPCHK( hipMemsetAsync( slow_word( ctx, 0 ), 0, FD_SW_CNT * sizeof(u32), ctx->stream ), -1 );
  fdgpu_debug_opts_t dbg; debug_opts_get( &dbg );   /* test / A/B choices (fdgpu_debug_set_opts), never the environment */
  ctx->half = dbg.half >= 0 ? dbg.half : FD_HALF;
  ctx->half_force_slow = dbg.half_force_slow;
  if( ctx->half ) {
    HIPCHK( ctx_dev_alloc( ctx, &ctx->d_tabR, ns * FD_ATAB_STORED * 8 * sizeof(uint4) ), -1 );
    HIPCHK( ctx_dev_alloc( ctx, &ctx->d_digR, ns * FD_HDIG ), -1 );
    HIPCHK( ctx_dev_alloc( ctx, &ctx->d_htop, ns ), -1 );
    HIPCHK( ctx_dev_alloc( ctx, &ctx->d_btab2, FD_BTAB_ENTRIES * 6 * sizeof(uint4) ), -1 );
    /* distinct keys decoded once (the decode lanes build the tables) */
    ctx->key_dedup = dbg.key_dedup != 1;
    if( ctx->key_dedup ) {
      unsigned long slots = 64UL;                    /* fdgpu_debug_opts_t.key_dedup = 2 (tests): 64 slots, 2 probes */
      if( dbg.key_dedup != 2 ) while( slots < 2UL*ns && slots < ( 1UL << 31 ) ) slots <<= 1;
      ctx->kd_slots = (u32)slots; ctx->kd_tiny = dbg.key_dedup == 2; ctx->kd_probes = ctx->kd_tiny ? 2u : FD_KD_PROBES;
      ctx->kd_seed = 0u;
      /* the fixed-base keys' choices (below), ahead of the table: the key cache's per-batch index lies in front of it,
         so that one memset clears both.  fdgpu_debug_opts_t.key_cache = 2 (tests): 8 slots, 8 words, 2 probes */
      ctx->key_fixed = dbg.key_split != 1 && dbg.key_fixed != 1 && !ctx->half_force_slow;
      if( ctx->key_fixed ) {
        ctx->fb_min = dbg.key_fixed == 2 ? 4u : FD_FB_MIN;
        unsigned long fc = ns / ctx->fb_min;
        ctx->fb_cap = (u32)( fc < FD_FB_CAP ? fc : FD_FB_CAP );
        ctx->kc_mode = dbg.key_cache; ctx->kc_dirty = 0; ctx->kc_batch = 0u;
        if( ctx->kc_mode == 2 && ctx->fb_cap > 8u ) ctx->fb_cap = 8u;
        u32 iw = 8u;
        if( ctx->kc_mode != 2 ) while( iw < 4u * ctx->fb_cap ) iw <<= 1;
        ctx->kc_iwords = iw; ctx->kc_iprobes = ctx->kc_mode == 2 ? 2u : FD_KD_PROBES;
        /* full slots: a batch promotes at most a quarter of the slots, which bounds its one-off cost */
        ctx->kfull_mode = dbg.key_full;
        ctx->pmax = ctx->kfull_mode == 1 ? 0u : ctx->fb_cap / 4u > 1u ? ctx->fb_cap / 4u : 1u;
        /* wide tables: the first wcap slots get them with their byte tables of groups 1..3 */
        ctx->wcap = dbg.key_wide == 1 ? 0u : dbg.key_wide == 2 ? ctx->fb_cap / 2u
                  : ctx->fb_cap < (u32)FD_FB_WCAP ? ctx->fb_cap : (u32)FD_FB_WCAP;
      }
      HIPCHK( ctx_dev_alloc( ctx, &ctx->d_kidx, ( (size_t)ctx->kc_iwords + slots ) * sizeof(u32) ), -1 );   /* (cleared per batch, */
      ctx->d_ktab = ctx->d_kidx + ctx->kc_iwords;                                                        /*  launch_half) */
      HIPCHK( ctx_dev_alloc( ctx, &ctx->d_arep, ns * sizeof(u32) ), -1 );
      HIPCHK( ctx_dev_alloc( ctx, &ctx->d_ulist, ns * sizeof(u32) ), -1 );
      HIPCHK( ctx_dev_alloc( ctx, &ctx->d_astat, ns ), -1 );
      /* the signatures of repeated keys walk 64 doublings (fd_keysplit_kernel) */
      ctx->key_split = dbg.key_split != 1;
      if( ctx->key_split ) {
        ctx->hot_min = dbg.key_split == 2 ? 2u : FD_HOT_MIN;
        ctx->hot_cap = (u32)( ns / ctx->hot_min );
        size_t hc = ctx->hot_cap ? ctx->hot_cap : 1UL;
        HIPCHK( ctx_dev_alloc( ctx, &ctx->d_kcnt, ns * sizeof(u32) ), -1 );
        HIPCHK( ctx_dev_alloc( ctx, &ctx->d_hidx, ns * sizeof(u32) ), -1 );
        HIPCHK( ctx_dev_alloc( ctx, &ctx->d_hlist, hc * sizeof(u32) ), -1 );
        HIPCHK( ctx_dev_alloc( ctx, &ctx->d_order, ns * sizeof(u32) ), -1 );
        HIPCHK( ctx_dev_alloc( ctx, &ctx->d_htab, hc * 2 * FD_ATAB_STORED * 8 * sizeof(uint4) ), -1 );
        HIPCHK( ctx_dev_alloc( ctx, &ctx->d_btabh, (size_t)3 * FD_BTAB_ENTRIES * 6 * sizeof(uint4) ), -1 );
        /* the keys with many signatures get fixed-base tables (fd_keyclass_kernel) */
        /* (not under half_force_slow: that hook sends signatures down the half-size slow list, which a fixed-base
           signature never sees) */
        if( ctx->key_fixed ) {                          /* (fb_min, fb_cap and the key cache's choices: set above) */
          size_t fcn = ctx->fb_cap ? ctx->fb_cap : 1UL;
          HIPCHK( ctx_dev_alloc( ctx, &ctx->d_fidx, ns * sizeof(u32) ), -1 );
          HIPCHK( ctx_dev_alloc( ctx, &ctx->d_flist, fcn * 2 * sizeof(u32) ), -1 );
          HIPCHK( ctx_dev_alloc( ctx, &ctx->d_skey, fcn * 8 * sizeof(u32) ), -1 );
          HIPCHK( ctx_dev_alloc( ctx, &ctx->d_sstate, fcn * 3 * sizeof(u32) ), -1 );
          ctx->d_sbirth = ctx->d_sstate + fcn; ctx->d_sfull = ctx->d_sbirth + fcn;
          HIPCHK( ctx_dev_alloc( ctx, &ctx->d_plist, ( ctx->pmax ? ctx->pmax : 1UL ) * sizeof(u32) ), -1 );
          HIPCHK( ctx_dev_alloc( ctx, &ctx->d_sstat, fcn ), -1 );
          HIPCHK( ctx_dev_alloc( ctx, &ctx->d_mlist, ( ns / ctx->fb_min + 1UL ) * sizeof(u32) ), -1 );
          HIPCHK( hipMemsetAsync( ctx->d_sstate, 0, fcn * 3 * sizeof(u32), ctx->stream ), -1 );   /* every slot empty */
          HIPCHK( ctx_dev_alloc( ctx, &ctx->d_orderh, ns * sizeof(u32) ), -1 );
          HIPCHK( ctx_dev_alloc( ctx, &ctx->d_fbase, fcn * FD_FB_NT * 8 * sizeof(uint4) ), -1 );
          HIPCHK( ctx_dev_alloc( ctx, &ctx->d_ftab, fcn * FD_FB_NT * FD_FB_E * 6 * sizeof(uint4) ), -1 );
          if( ctx->wcap ) {
            HIPCHK( ctx_dev_alloc( ctx, &ctx->d_wbase, (size_t)ctx->wcap * 16 * 8 * sizeof(uint4) ), -1 );
            HIPCHK( ctx_dev_alloc( ctx, &ctx->d_wtab, ( (size_t)ctx->wcap * 8 * FD_FB_WE + 1 ) * 6 * sizeof(uint4) ), -1 );
            HIPCHK( hipMemcpyAsync( ctx->d_wtab, fd_ptab_ident_host, sizeof(fd_ptab_ident_host), hipMemcpyHostToDevice, ctx->stream ), -1 );
          }
          HIPCHK( ctx_dev_alloc( ctx, &ctx->d_btabf, (size_t)FD_FB_NB * FD_BTAB_ENTRIES * 6 * sizeof(uint4) ), -1 );
          HIPCHK( ctx_dev_alloc( ctx, &ctx->d_fslow, ns * sizeof(u32) ), -1 );
        }
      }
    }
  }
  ctx->small_max  = dbg.small_batch_max >= 0 ? (unsigned long)dbg.small_batch_max : FD_SMALL_BATCH_MAX;
  ctx->dsm_lanes  = dbg.dsm_lanes;
  ctx->nofold_max = dbg.nofold_max >= 0 ? (unsigned long)dbg.nofold_max : FD_NOFOLD_MAX;
  ctx->gather_nowb = dbg.gather_no_writeback;
  ctx->poll_pf = dbg.poll_prefetch > 0 ? dbg.poll_prefetch : 0;
  ctx->gather_rpb = dbg.gather_rpb == 1 ? 1 : 4;
  ctx->gather_cu_spread = dbg.gather_cu_spread;
  ctx->quad_sha = dbg.quad_sha;
  for( int i=0; i<5; i++ ) HIPCHK( hipEventCreate( &ctx->ev[i] ), -1 );
  for( int r=0; r<FD_NRING; r++ ) for( int i=0; i<5; i++ ) HIPCHK( hipEventCreate( &ctx->ring[r][i] ), -1 );
  ctx->ring_cnt = 0;
  hipLaunchKernelGGL( fd_btab_kernel, dim3((FD_BTAB_ENTRIES + 255)/256), dim3(256), 0, ctx->stream, ctx->d_btab, 0 );
  if( ctx->half )
    hipLaunchKernelGGL( fd_btab_kernel, dim3((FD_BTAB_ENTRIES + 255)/256), dim3(256), 0, ctx->stream, ctx->d_btab2, 120 );
  if( ctx->key_split ) {
    int const e[ 3 ] = { 72, 140, 196 };               /* the hot walk's s' digits 5-8, 9-12, 13-15 (hs_hot_bwin) */
    for( int t=0; t<3; t++ )
      hipLaunchKernelGGL( fd_btab_kernel, dim3((FD_BTAB_ENTRIES + 255)/256), dim3(256), 0, ctx->stream,
                          ctx->d_btabh + (size_t)t * FD_BTAB_ENTRIES * 6, e[t] );
  }
  if( ctx->key_fixed )
    for( int u=0; u<FD_FB_NB; u++ )                    /* (the walk with doublings reads the even ones) */
      hipLaunchKernelGGL( fd_btab_kernel, dim3((FD_BTAB_ENTRIES + 255)/256), dim3(256), 0, ctx->stream,
                          ctx->d_btabf + (size_t)u * FD_BTAB_ENTRIES * 6, 16*u );
  HIPCHK( hipGetLastError(), -1 );
  for( int i=0; i<FD_NSLOT; i++ ) HIPCHK( hipEventCreateWithFlags( &ctx->slot[i].done, hipEventDisableTiming ), -1 );
  HIPCHK( ctx_pin_alloc( ctx, &ctx->h_flag, ( FD_NSLOT + 2 ) * sizeof(unsigned long), &ctx->d_flag ), -1 );
  for( int i=0; i<=FD_NSLOT+1; i++ ) ctx->h_flag[i] = 0UL;   /* [FD_NSLOT]: stream_wait's word, [FD_NSLOT+1]: gathers */
  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_gcnt, sizeof(unsigned long) ), -1 );
  HIPCHK( hipMemsetAsync( ctx->d_gcnt, 0, sizeof(unsigned long), ctx->stream ), -1 );
  HIPCHK( ctx_pin_alloc( ctx, &ctx->h_stamp, ( 2*FD_NSLOT + 1 ) * sizeof(unsigned long), &ctx->d_stamp ), -1 );
  memset( ctx->h_stamp, 0, ( 2*FD_NSLOT + 1 ) * sizeof(unsigned long) );
  ctx->last_gt = -1;
  if( dbg.cu_exclusive > 0 && fdgpu_ed25519_set_cu_exclusive( ctx, dbg.cu_exclusive ) ) return -1;
  if( dbg.cu_exclusive < 0 ) ctx->excl_mode = -1;      /* explicitly off: a verify tile keeps it off too */
  /* slot 0 now (the synchronous host calls stage through it); the async
     pipeline's other slots on first use (slot_bufs) */
  if( max_payload_bytes && slot_bufs( ctx, 0 ) ) return -1;
  ctx->cur = 0; ctx->rec_fp_off = -1;
  HIPCHK( hipStreamSynchronize( ctx->stream ), -1 );
  gclk_calibrate( ctx );
  return 0;
}

extern "C" void fdgpu_ed25519_set_timing( fdgpu_ed25519_ctx_t * ctx, int enable ) { ctx->timing = enable; ctx->ring_cnt = 0; }

/* mean duration of kernel idx over the batches launched since timing was
   enabled (at most the last FD_NRING), from HIP events recorded on the
   stream the kernels ran on */
extern "C" float
fdgpu_ed25519_kernel_ms( fdgpu_ed25519_ctx_t * ctx, int idx ) {
  if( idx<0 || idx>4 || !ctx->ring_cnt ) return -1.f;
  unsigned long n = ctx->ring_cnt < (unsigned long)FD_NRING ? ctx->ring_cnt : (unsigned long)FD_NRING;
  /* 0 prep, 1 walk, 2 reduce; throughput path's prep split: 3 the decode kernel, 4 the hash (+ table) kernels */
  static int const from[5] = { 0, 1, 2, 0, 4 }, to[5] = { 1, 2, 3, 4, 1 };
  double sum = 0.;
  for( unsigned long r=0; r<n; r++ ) {
    float ms = 0.f;
    if( hipEventElapsedTime( &ms, ctx->ring[r][ from[idx] ], ctx->ring[r][ to[idx] ] ) != hipSuccess ) return -1.f;
    sum += ms;
  }
  return (float)( sum / (double)n );
}

/* ---- VALU integer peak probe --------------------------------------------
   Sustained v_mad_u64_u32 rate of this device: 16 independent 64-bit
   accumulator chains per lane (no memory traffic), full grid.  This is the
   "peak" the prep/dsm kernels' multiply-accumulate count is priced against
   (MI355X_MICROARCH.md has no integer-multiply row). */
__global__ void __launch_bounds__( 256 )
fd_mad_probe_kernel( u32 iters, u32 seed, u64 * out ) {
  u64 acc[16]; u32 a = seed + threadIdx.x, b = seed ^ (blockIdx.x * 2654435761u);
#pragma unroll
  for( int i=0; i<16; i++ ) acc[i] = (u64)(a + i) << 7;
  for( u32 it=0; it<iters; it++ ) {
#pragma unroll
    for( int i=0; i<16; i++ ) {
      asm volatile( "v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc[i]) : "v"(a), "v"(b) : "vcc" );
    }
  }
  u64 x = 0;
#pragma unroll
  for( int i=0; i<16; i++ ) x ^= acc[i];
  if( x == 0x1234567ull ) out[0] = x;
}

extern "C" double
fdgpu_mad_peak_per_s( int device ) {
  if( hipSetDevice( device ) != hipSuccess ) return -1.;
  hipDeviceProp_t prop; hipGetDeviceProperties( &prop, device );
  int grid = prop.multiProcessorCount * 8;   /* 8 x 256 threads per CU = 8 waves/SIMD */
  u64 * d_out; hipMalloc( &d_out, 8 );
  hipEvent_t e0, e1; hipEventCreate( &e0 ); hipEventCreate( &e1 );
  u32 iters = 16384;
  hipLaunchKernelGGL( fd_mad_probe_kernel, dim3(grid), dim3(256), 0, 0, 16u, 1u, d_out );
  hipEventRecord( e0, 0 );
  hipLaunchKernelGGL( fd_mad_probe_kernel, dim3(grid), dim3(256), 0, 0, iters, 1u, d_out );
  hipEventRecord( e1, 0 );
  hipEventSynchronize( e1 );
  float ms = 0.f; hipEventElapsedTime( &ms, e0, e1 );
  hipEventDestroy( e0 ); hipEventDestroy( e1 ); hipFree( d_out );
  double macs = (double)grid * 256. * 16. * (double)iters;
  return ms > 0.f ? macs / ( (double)ms * 1e-3 ) : -1.;
}

extern "C" int
fdgpu_ed25519_verify_txns_device( fdgpu_ed25519_ctx_t * ctx, unsigned char const * d_payload,
                                  fdgpu_txn_desc_t const * d_desc, unsigned long txn_cnt, unsigned long sig_cnt,
                                  signed char * d_txn_out, signed char * d_sig_out, void * stream ) {
  if( !ctx ) { fd_err = "NULL ctx"; return -1; }
  if( txn_cnt > ctx->max_txn || sig_cnt > ctx->max_sig ) { fd_err = "batch larger than ctx"; return -1; }
  HIPCHK( hipSetDevice( ctx->device ), -2 );
  return launch_batch( ctx, d_payload, d_desc, txn_cnt, sig_cnt, (i8*)d_txn_out, (i8*)d_sig_out,
                       stream ? (hipStream_t)stream : ctx->stream );
}

/* Host regions the GPU may read or write directly (fdgpu_host_alloc
   allocations and fdgpu_host_register-ed ranges): host base -> device
   address, for the gather path and for payloads the host calls read in place. */
/* A fixed table read without a lock (every tile thread looks its frags up
   here in during_frag; a global mutex there was contended by all of them):
   writers (register / unregister, rare) serialise on a mutex, fill an
   entry's fields and then publish it with a release store of its size; a
   removed entry's size drops to 0 first. */
#define FD_REGION_MAX 256
struct fd_region { unsigned char const * h; unsigned char * d; std::atomic<unsigned long> sz; int refs, shared; };
static std::mutex g_reg_mu;
static fd_region g_regions[ FD_REGION_MAX ];
static std::atomic<int> g_region_cnt{ 0 };

/* device address of [p, p+sz) if it lies inside one registered region, else NULL */
static unsigned char * region_dev( void const * p, unsigned long sz ) {
  unsigned char const * q = (unsigned char const *)p;
  /* a tile's frags come from one region: try the thread's last hit first (re-validated like
     any entry, so a removed or reused entry is never trusted) */
  static thread_local int hint = 0;
  int n = g_region_cnt.load( std::memory_order_acquire );
  if( hint < n ) {
    unsigned long rs = g_regions[hint].sz.load( std::memory_order_acquire );
    unsigned char const * h = g_regions[hint].h;
    if( rs && q >= h && q + sz <= h + rs ) return g_regions[hint].d + ( q - h );
  }
  for( int i=0; i<n; i++ ) {
    unsigned long rs = g_regions[i].sz.load( std::memory_order_acquire );
    unsigned char const * h = g_regions[i].h;
    if( rs && q >= h && q + sz <= h + rs ) { hint = i; return g_regions[i].d + ( q - h ); }
  }
  return NULL;
}

/* Host-side validation of a batch before staging: payload bounds and
   the sig_base prefix (the device kernels additionally bound-check every
   transaction against its own payload). */
static int check_batch( fdgpu_txn_desc_t const * desc, unsigned long txn_cnt, unsigned long payload_bytes,
                        unsigned long * sig_total ) {
  unsigned long s = 0;
  for( unsigned long i=0; i<txn_cnt; i++ ) {
    if( desc[i].sig_base != s ) { fd_err = "sig_base is not the prefix sum of sig_cnt"; return -1; }
    if( (unsigned long)desc[i].payload_off + desc[i].payload_sz > payload_bytes ) { fd_err = "payload out of arena"; return -1; }
    s += desc[i].sig_cnt;
  }
  *sig_total = s;
  return 0;
}

/* What the synchronous host calls share.  sync_ctx: is there a context (and, for the calls that pack
   records into it, a staging slot)?  sync_begin, once the call's own arguments are checked: the calls
   stage through slot 0, so only while the async pipeline holds nothing.  sync_finish: slot 0's
   transaction codes (and the signature codes, if asked for) back to the caller, behind everything queued
   on the context's stream; pageable = 1 if the call queued a copy into pageable host memory (stream_wait). */
static int sync_ctx( fdgpu_ed25519_ctx_t const * ctx, int staged ) {
  if( !ctx ) { fd_err = "NULL ctx"; return -1; }
  if( staged && !ctx->slot[0].h_payload ) { fd_err = "ctx has no staging buffers (max_payload_bytes==0)"; return -3; }
  return 0;
}
static int sync_begin( fdgpu_ed25519_ctx_t * ctx ) {
  HIPCHK( hipSetDevice( ctx->device ), -2 );
  if( async_busy( ctx ) ) { fd_err = "async batches pending or in flight"; return -1; }
  return 0;
}
static int sync_finish( fdgpu_ed25519_ctx_t * ctx, unsigned long txn_cnt, signed char * txn_out,
                        signed char * sig_out, unsigned long nsig, int pageable ) {
  fd_slot & sl = ctx->slot[0];
  hipStream_t st = ctx->stream;
  HIPCHK( hipMemcpyAsync( sl.h_txn_out, sl.d_txn_out, txn_cnt, hipMemcpyDeviceToHost, st ), -2 );
  if( sig_out && nsig ) HIPCHK( hipMemcpyAsync( sig_out, ctx->d_code, nsig, hipMemcpyDeviceToHost, st ), -2 );
  if( stream_wait( ctx, st, pageable || ( sig_out && nsig ) ) ) return -2;
  memcpy( txn_out, sl.h_txn_out, txn_cnt );
  return 0;
}

/* Large host batches: sub-batches of ~FD_PIPE_SUB transactions.  The
   payload bytes of sub-batch i go up on the copy stream (straight from a
   pinned region, or through the pinned staging slot) while the kernels of
   sub-batch i-1 run on the compute stream, which waits for copy i by an
   event.  Only the compute stream waits, and only on copies enqueued
   before the wait; the copy stream never waits (no write-after-read on
   its buffers: every sub-batch has its own range of one arena), so no
   cycle of cross-queue waits can form whatever hardware queues the two
   streams share. */
static int
verify_host_pipelined( fdgpu_ed25519_ctx_t * ctx, unsigned char const * payload, unsigned long payload_bytes,
                       fdgpu_txn_desc_t const * desc, unsigned long txn_cnt, unsigned long nsig,
                       signed char * txn_out, signed char * sig_out ) {
  fd_slot & sl = ctx->slot[0];
  if( !ctx->cstream ) {
    /* created on first use: every stream of the process takes a place in the runtime's
       stream -> hardware queue assignment, and the tiles' contexts never need this one */
    HIPCHK( hipStreamCreateWithFlags( &ctx->cstream, hipStreamNonBlocking ), -2 );
    for( unsigned long i=0; i<FD_PIPE_MAX; i++ ) HIPCHK( hipEventCreateWithFlags( &ctx->pipe_ev[i], hipEventDisableTiming ), -2 );
  }
  hipStream_t st = ctx->stream, cs = ctx->cstream;
  unsigned long nsub = txn_cnt / FD_PIPE_SUB;
  if( nsub > FD_PIPE_MAX ) nsub = FD_PIPE_MAX;
  int pinned = region_dev( payload, payload_bytes ) != NULL;
  /* descriptors with each sub-batch's sig_base rebased to its first signature */
  unsigned long sig_lo[ FD_PIPE_MAX + 1 ], txn_lo[ FD_PIPE_MAX + 1 ];
  for( unsigned long i=0; i<=nsub; i++ ) txn_lo[i] = txn_cnt * i / nsub;
  for( unsigned long i=0; i<nsub; i++ ) {
    sig_lo[i] = desc[ txn_lo[i] ].sig_base;
    for( unsigned long t=txn_lo[i]; t<txn_lo[i+1]; t++ ) { sl.h_desc[t] = desc[t]; sl.h_desc[t].sig_base -= (unsigned)sig_lo[i]; }
  }
  sig_lo[nsub] = nsig;
  HIPCHK( hipMemcpyAsync( sl.d_desc, sl.h_desc, txn_cnt * sizeof(fdgpu_txn_desc_t), hipMemcpyHostToDevice, cs ), -2 );
  HIPCHK( hipMemsetAsync( sl.d_payload + payload_bytes, 0, FD_ARENA_SLACK, cs ), -2 );
  for( unsigned long i=0; i<nsub; i++ ) {
    unsigned long lo = ~0UL, hi = 0UL;
    for( unsigned long t=txn_lo[i]; t<txn_lo[i+1]; t++ ) {
      unsigned long a = desc[t].payload_off, b = a + desc[t].payload_sz;
      if( a < lo ) lo = a;
      if( b > hi ) hi = b;
    }
    if( hi > lo ) {
      unsigned char const * src = payload + lo;
      if( !pinned ) { memcpy( sl.h_payload + lo, payload + lo, hi - lo ); src = sl.h_payload + lo; }
      HIPCHK( hipMemcpyAsync( sl.d_payload + lo, src, hi - lo, hipMemcpyHostToDevice, cs ), -2 );
    }
    HIPCHK( hipEventRecord( ctx->pipe_ev[i], cs ), -2 );
    HIPCHK( hipStreamWaitEvent( st, ctx->pipe_ev[i], 0 ), -2 );
    int rc = launch_batch( ctx, sl.d_payload, sl.d_desc + txn_lo[i], txn_lo[i+1] - txn_lo[i], sig_lo[i+1] - sig_lo[i],
                           sl.d_txn_out + txn_lo[i], ctx->d_code + sig_lo[i], st );
    if( rc ) return rc;
  }
  return sync_finish( ctx, txn_cnt, txn_out, sig_out, nsig, 0 );
}

extern "C" int
fdgpu_ed25519_verify_txns_host( fdgpu_ed25519_ctx_t * ctx, unsigned char const * payload, unsigned long payload_bytes,
                                fdgpu_txn_desc_t const * desc, unsigned long txn_cnt,
                                signed char * txn_out, signed char * sig_out ) {
  int rc = sync_ctx( ctx, 0 );
  if( rc ) return rc;
  unsigned long nsig;
  if( check_batch( desc, txn_cnt, payload_bytes, &nsig ) ) return -1;
  if( txn_cnt > ctx->max_txn || nsig > ctx->max_sig || payload_bytes > ctx->max_payload ) { fd_err = "batch larger than ctx"; return -1; }
  if( !txn_cnt ) return 0;
  if( ( rc = sync_begin( ctx ) ) ) return rc;
  fd_slot & sl = ctx->slot[0];
  hipStream_t st = ctx->stream;
  if( txn_cnt >= 2UL*FD_PIPE_SUB ) return verify_host_pipelined( ctx, payload, payload_bytes, desc, txn_cnt, nsig, txn_out, sig_out );
  memcpy( sl.h_desc, desc, txn_cnt * sizeof(fdgpu_txn_desc_t) );
  HIPCHK( hipMemcpyAsync( sl.d_desc, sl.h_desc, txn_cnt * sizeof(fdgpu_txn_desc_t), hipMemcpyHostToDevice, st ), -2 );
  if( region_dev( payload, payload_bytes ) ) {
    /* the caller's payload is already pinned (fdgpu_host_alloc / fdgpu_host_register, e.g. a
       registered dcache): one DMA straight from it, no staging copy; the slack is zeroed on the device */
    HIPCHK( hipMemcpyAsync( sl.d_payload, payload, payload_bytes, hipMemcpyHostToDevice, st ), -2 );
    HIPCHK( hipMemsetAsync( sl.d_payload + payload_bytes, 0, FD_ARENA_SLACK, st ), -2 );
  } else {
  /* stage in chunks: the DMA of chunk i overlaps the host copy of chunk i+1 */
  memset( sl.h_payload + payload_bytes, 0, FD_ARENA_SLACK );
  for( unsigned long off=0UL; off<payload_bytes+FD_ARENA_SLACK; off+=FD_STAGE_CHUNK ) {
    unsigned long end = off + FD_STAGE_CHUNK < payload_bytes + FD_ARENA_SLACK ? off + FD_STAGE_CHUNK : payload_bytes + FD_ARENA_SLACK;
    if( off < payload_bytes ) memcpy( sl.h_payload + off, payload + off, ( end < payload_bytes ? end : payload_bytes ) - off );
    HIPCHK( hipMemcpyAsync( sl.d_payload + off, sl.h_payload + off, end - off, hipMemcpyHostToDevice, st ), -2 );
  }
  }
  if( ( rc = launch_batch( ctx, sl.d_payload, sl.d_desc, txn_cnt, nsig, sl.d_txn_out, NULL, st ) ) ) return rc;
  return sync_finish( ctx, txn_cnt, txn_out, sig_out, nsig, 0 );
}

/* Records scattered in host memory, verified through slot 0 in chunks of up to max_txn transactions /
   max_sig signatures / max_payload bytes (the caller has checked that each record alone fits).
   desc_of( i ) gives record i's descriptor -- its payload_off and sig_base are set here -- and
   pack( i, dst ) writes its payload_sz bytes; out[i] gets its code. */
template< class D, class P > static int
verify_chunks( fdgpu_ed25519_ctx_t * ctx, unsigned long cnt, signed char * out, D desc_of, P pack ) {
  fd_slot & sl = ctx->slot[0];
  hipStream_t st = ctx->stream;
  unsigned long done = 0;
  while( done < cnt ) {
    unsigned long n = 0, nsig = 0; size_t used = 0;
    while( done + n < cnt && n < ctx->max_txn ) {
      fdgpu_txn_desc_t d = desc_of( done + n );
      if( used + d.payload_sz + 8UL > ctx->max_payload || nsig + d.sig_cnt > ctx->max_sig ) break;
      pack( done + n, sl.h_payload + used );
      d.payload_off = (unsigned)used; d.sig_base = (unsigned)nsig;
      sl.h_desc[n] = d;
      used = ( used + d.payload_sz + 7UL ) & ~(size_t)7; nsig += d.sig_cnt; n++;
    }
    memset( sl.h_payload + used, 0, FD_ARENA_SLACK );
    HIPCHK( hipMemcpyAsync( sl.d_payload, sl.h_payload, used + FD_ARENA_SLACK, hipMemcpyHostToDevice, st ), -2 );
    HIPCHK( hipMemcpyAsync( sl.d_desc, sl.h_desc, n * sizeof(fdgpu_txn_desc_t), hipMemcpyHostToDevice, st ), -2 );
    int rc = launch_batch( ctx, sl.d_payload, sl.d_desc, n, nsig, sl.d_txn_out, NULL, st );
    if( rc ) return rc;
    if( ( rc = sync_finish( ctx, n, out + done, NULL, 0UL, 0 ) ) ) return rc;
    done += n;
  }
  return 0;
}

/* A (msg, sig, pub) triple as a one-signer transaction: its descriptor, and its bytes sig | pub | msg */
static fdgpu_txn_desc_t
one_signer_desc( unsigned long msg_sz ) {
  fdgpu_txn_desc_t d = {};
  d.payload_sz = (unsigned short)( 96UL + msg_sz );
  d.message_off = 96; d.acct_addr_off = 64; d.signature_off = 0; d.sig_cnt = 1;
  return d;
}
static void
pack_triple( unsigned char * dst, unsigned char const * sig, unsigned char const * pub, unsigned char const * msg,
             unsigned long msg_sz ) {
  memcpy( dst, sig, 64 ); memcpy( dst + 64, pub, 32 );
  if( msg_sz ) memcpy( dst + 96, msg, msg_sz );
}

/* Independent (msg, sig, pub) triples -- the batched form of
   fd_ed25519_verify for callers that verify unrelated messages (gossip
   CRDS values and ping/pong, fd_gossvf_tile.c:367-446; precompiles).
   Each triple is packed sig | pub | msg into the staging arena as a
   one-signer transaction; chunks of up to max_txn triples. */
extern "C" int
fdgpu_ed25519_verify_many_host( fdgpu_ed25519_ctx_t * ctx, unsigned char const * const * msgs,
                                unsigned long const * msg_szs, unsigned char const * const * sigs,
                                unsigned char const * const * pubs, unsigned long cnt, signed char * out ) {
  int rc = sync_ctx( ctx, 1 );
  if( rc || ( rc = sync_begin( ctx ) ) ) return rc;
  for( unsigned long i=0; i<cnt; i++ )
    if( msg_szs[i] > 0xffffUL - 96UL || 96UL + msg_szs[i] + 8UL > ctx->max_payload ) { fd_err = "message too long"; return -1; }
  return verify_chunks( ctx, cnt, out,
    [&]( unsigned long i ) { return one_signer_desc( msg_szs[i] ); },
    [&]( unsigned long i, unsigned char * b ) { pack_triple( b, sigs[i], pubs[i], msgs[i], msg_szs[i] ); } );
}

/* Transactions scattered in host memory, each already parsed (the replay
   path: fd_executor_txn_verify, src/flamenco/runtime/fd_executor.c:
   1550-1574, once per transaction of a block, each over its own
   txn_ctx->_txn_raw->raw).  desc[i] holds transaction i's fd_txn_t fields
   (signature_off, acct_addr_off, message_off, sig_cnt) and payload_sz;
   payload_off / sig_base are ignored.  out[i] = the
   fd_ed25519_verify_batch_single_msg code of transaction i.  Chunks of up
   to max_txn transactions / max_sig signatures / max_payload bytes. */
extern "C" int
fdgpu_ed25519_verify_txn_ptrs( fdgpu_ed25519_ctx_t * ctx, unsigned char const * const * payloads,
                               fdgpu_txn_desc_t const * desc, unsigned long cnt, signed char * out ) {
  int rc = sync_ctx( ctx, 1 );
  if( rc || ( rc = sync_begin( ctx ) ) ) return rc;
  for( unsigned long i=0; i<cnt; i++ )
    if( (unsigned long)desc[i].payload_sz + 8UL > ctx->max_payload || desc[i].sig_cnt > ctx->max_sig ) {
      fd_err = "transaction larger than the ctx"; return -1;
    }
  return verify_chunks( ctx, cnt, out,
    [&]( unsigned long i ) { return desc[i]; },
    [&]( unsigned long i, unsigned char * b ) { memcpy( b, payloads[i], desc[i].payload_sz ); } );
}

/* ---- per-signature descriptors ------------------------------ */

/* What every entry point of the descriptor front-ends refuses first, like HIPCHK by returning: no
   context, then a faulted one; and, where the call needs it, a context that `prepare` has not prepared (cap: the
   prepared size, 0 = none).  Behind them a call checks its sizes, returns 0 for no records, refuses a NULL and then
   a misaligned argument, in this order. */
#define FRONT_CTX( ctx ) do { if( !(ctx) ) { fd_err = "NULL ctx"; return -1; }                                           \
    if( (ctx)->fault ) { fd_err = std::string( __func__ ) + ": the context has faulted"; return -3; } } while(0)
#define FRONT_PREPARED( cap, prepare ) do { if( !(cap) ) { fd_err = std::string( __func__ ) + ": no " prepare; return -3; } } while(0)

extern "C" int
fdgpu_ed25519_sigs_prepare( fdgpu_ed25519_ctx_t * ctx, unsigned long max_packed_bytes ) {
  FRONT_CTX( ctx );
  if( max_packed_bytes < FD_SIG_DESC_HDR || max_packed_bytes + FD_ARENA_SLACK > ( 1UL << 32 ) ) {
    fd_err = "fdgpu_ed25519_sigs_prepare: bad size"; return -1;
  }
  HIPCHK( hipSetDevice( ctx->device ), -2 );
  size_t ns = ctx->max_sig;
  if( !ctx->d_sg_btot ) {              /* (the last one allocated: all of them or none) */
    HIPCHK( ctx_dev_alloc( ctx, &ctx->d_sg_tdesc, ns * sizeof(fdgpu_txn_desc_t) ), -2 );
    HIPCHK( ctx_dev_alloc( ctx, &ctx->d_sg_desc, ns * sizeof(fdgpu_sig_desc_t) ), -2 );
    HIPCHK( ctx_dev_alloc( ctx, &ctx->d_sg_loc, ns * sizeof(u32) ), -2 );
    HIPCHK( ctx_dev_alloc( ctx, &ctx->d_sg_flag, ns ), -2 );
    HIPCHK( ctx_dev_alloc( ctx, &ctx->d_sg_out, ns ), -2 );
    HIPCHK( ctx_dev_alloc( ctx, &ctx->d_sg_btot, ( ns / FD_WG + 1UL ) * sizeof(unsigned long) ), -2 );
  }
  if( max_packed_bytes <= ctx->sg_cap ) return 0;
  /* a larger arena: nothing of the context may still read the old one */
  HIPCHK( hipDeviceSynchronize(), -2 );
  ctx->sg_cap = 0UL;
  ctx_dev_free( ctx, &ctx->d_sg_pack );
  size_t bytes = max_packed_bytes + 2UL * FD_ARENA_SLACK;
  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_sg_pack, bytes ), -2 );
  HIPCHK( hipMemsetAsync( ctx->d_sg_pack, 0, bytes, ctx->stream ), -2 );
  HIPCHK( hipStreamSynchronize( ctx->stream ), -2 );
  ctx->sg_cap = max_packed_bytes;
  return 0;
}

/* the kernels of one batch of descriptors on st: size, scan, place, pack, the batch itself, the flags */
static int
sigs_launch( fdgpu_ed25519_ctx_t * ctx, unsigned char const * d_arena, unsigned long arena_sz,
             fdgpu_sig_desc_t const * d_desc, unsigned long cnt, i8 * d_out, hipStream_t st ) {
  u32 n = (u32)cnt;
  unsigned nb = (unsigned)( ( cnt + FD_WG - 1 ) / FD_WG );
  hipLaunchKernelGGL( fd_sig_size_kernel, dim3(nb), dim3(FD_WG), 0, st, d_desc, n, arena_sz, ctx->d_sg_loc, ctx->d_sg_flag,
                      ctx->d_sg_btot );
  hipLaunchKernelGGL( fd_sig_scan_kernel, dim3(1), dim3(FD_WG), 0, st, ctx->d_sg_btot, (u32)nb );
  hipLaunchKernelGGL( fd_sig_place_kernel, dim3(nb), dim3(FD_WG), 0, st, d_desc, n, (u32 const *)ctx->d_sg_loc,
                      (unsigned long const *)ctx->d_sg_btot, ctx->sg_cap, ctx->d_sg_flag, ctx->d_sg_tdesc );
  hipLaunchKernelGGL( fd_sig_pack_kernel, dim3( (unsigned)( ( cnt + FD_SIG_RPB - 1 ) / FD_SIG_RPB ) ), dim3( 64 * FD_SIG_RPB ), 0, st,
                      d_arena, d_desc, (fdgpu_txn_desc_t const *)ctx->d_sg_tdesc, (unsigned char const *)ctx->d_sg_flag, n,
                      ctx->d_sg_pack );
  HIPCHK( hipGetLastError(), -3 );
  int rc = launch_batch( ctx, ctx->d_sg_pack, ctx->d_sg_tdesc, cnt, cnt, d_out, NULL, st );
  if( rc ) return rc;
  hipLaunchKernelGGL( fd_sig_flag_kernel, dim3(nb), dim3(FD_WG), 0, st, (unsigned char const *)ctx->d_sg_flag, n, d_out );
  HIPCHK( hipGetLastError(), -3 );
  return 0;
}

extern "C" int
fdgpu_ed25519_verify_sigs_device( fdgpu_ed25519_ctx_t * ctx, unsigned char const * d_arena, unsigned long arena_sz,
                                  fdgpu_sig_desc_t const * d_desc, unsigned long cnt, unsigned long msg_bytes,
                                  signed char * d_out, void * stream ) {
  FRONT_CTX( ctx ); FRONT_PREPARED( ctx->sg_cap, "fdgpu_ed25519_sigs_prepare" );
  if( cnt > ctx->max_sig || cnt > ctx->max_txn ) { fd_err = "batch larger than ctx"; return -1; }
  if( msg_bytes > ctx->sg_cap || 104UL * cnt > ctx->sg_cap - msg_bytes ) {
    fd_err = "fdgpu_ed25519_verify_sigs_device: 104 cnt + msg_bytes exceeds the prepared size"; return -1;
  }
  if( !cnt ) return 0;
  if( !d_arena || !d_desc || !d_out ) { fd_err = "NULL argument"; return -1; }
  HIPCHK( hipSetDevice( ctx->device ), -2 );
  return sigs_launch( ctx, d_arena, arena_sz, d_desc, cnt, (i8 *)d_out, stream ? (hipStream_t)stream : ctx->stream );
}

extern "C" int
fdgpu_ed25519_verify_sigs_host( fdgpu_ed25519_ctx_t * ctx, unsigned char const * arena, unsigned long arena_sz,
                                fdgpu_sig_desc_t const * desc, unsigned long cnt, signed char * out ) {
  FRONT_CTX( ctx );
  if( !cnt ) return 0;
  if( !arena || !desc || !out ) { fd_err = "NULL argument"; return -1; }
  int rc;
  unsigned char const * d_arena = region_dev( arena, arena_sz + FD_ARENA_SLACK );
  if( d_arena ) {
    /* in place: the GPU packs each chunk straight from the caller's region */
    FRONT_PREPARED( ctx->sg_cap, "fdgpu_ed25519_sigs_prepare" );
    if( ( rc = sync_begin( ctx ) ) ) return rc;
    hipStream_t st = ctx->stream;
    unsigned long most = ctx->max_sig < ctx->max_txn ? ctx->max_sig : ctx->max_txn;
    for( unsigned long done=0UL; done<cnt; ) {
      unsigned long n = 0UL, used = 0UL;
      while( done + n < cnt && n < most ) {
        fdgpu_sig_desc_t const & d = desc[ done + n ];
        int bad;
        unsigned long sz = fd_sig_desc_size( d.sig_off, d.pub_off, d.msg_off, d.msg_sz, arena_sz, &bad );
        if( used + sz > ctx->sg_cap ) break;
        used += sz; n++;
      }
      if( !n ) { fd_err = "fdgpu_ed25519_verify_sigs_host: a record larger than the prepared size"; return -1; }
      HIPCHK( hipMemcpyAsync( ctx->d_sg_desc, desc + done, n * sizeof(fdgpu_sig_desc_t), hipMemcpyHostToDevice, st ), -2 );
      if( ( rc = sigs_launch( ctx, d_arena, arena_sz, ctx->d_sg_desc, n, ctx->d_sg_out, st ) ) ) return rc;
      HIPCHK( hipMemcpyAsync( out + done, ctx->d_sg_out, n, hipMemcpyDeviceToHost, st ), -2 );
      if( stream_wait( ctx, st, 1 ) ) return -2;
      done += n;
    }
    return 0;
  }
  /* any other host memory: checked here, the good records packed through the staging slot as
     fdgpu_ed25519_verify_many_host packs its triples, run by run between the bad ones */
  if( ( rc = sync_ctx( ctx, 1 ) ) || ( rc = sync_begin( ctx ) ) ) return rc;
  for( unsigned long i=0UL; i<cnt; i++ ) {
    fdgpu_sig_desc_t const & d = desc[i];
    if( !fd_sig_desc_bad( d.sig_off, d.pub_off, d.msg_off, d.msg_sz, arena_sz ) && 96UL + d.msg_sz + 8UL > ctx->max_payload ) {
      fd_err = "message too long"; return -1;
    }
  }
  for( unsigned long i=0UL; i<cnt; ) {
    fdgpu_sig_desc_t const * r = desc + i;
    if( fd_sig_desc_bad( r->sig_off, r->pub_off, r->msg_off, r->msg_sz, arena_sz ) ) { out[i++] = (signed char)FDGPU_ERR_DESC; continue; }
    unsigned long m = 1UL;
    while( i + m < cnt && !fd_sig_desc_bad( r[m].sig_off, r[m].pub_off, r[m].msg_off, r[m].msg_sz, arena_sz ) ) m++;
    rc = verify_chunks( ctx, m, out + i,
      [&]( unsigned long k ) { return one_signer_desc( r[k].msg_sz ); },
      [&]( unsigned long k, unsigned char * b ) { pack_triple( b, arena + r[k].sig_off, arena + r[k].pub_off, arena + r[k].msg_off, r[k].msg_sz ); } );
    if( rc ) return rc;
    i += m;
  }
  return 0;
}

/* ---- Merkle shreds ------------------------------------------ */

#define FD_SHRED_STRIDE 1232UL     /* the host form's staging: a shred's first min( sz, 1228 ) bytes every 1,232 */

/* A front-end's device buffers grow in two steps, the caller's own buffers between them.  front_release: larger
   buffers, so nothing of the context may still read the old ones; unprepared, then they go.  front_prepare: buffers
   for records and keys, the pack zeroed, and only then prepared. */
static int
front_release( fdgpu_ed25519_ctx_t * ctx, fd_front * f ) {
  HIPCHK( hipDeviceSynchronize(), -2 );
  f->max = 0UL; f->keys = 0UL; f->sig = 0UL;
  ctx_dev_free( ctx, &f->d_pack ); ctx_dev_free( ctx, &f->d_tdesc ); ctx_dev_free( ctx, &f->d_code );
  ctx_dev_free( ctx, &f->d_flag ); ctx_dev_free( ctx, &f->d_out );   ctx_dev_free( ctx, &f->d_root );
  ctx_dev_free( ctx, &f->d_keys );
  return 0;
}
static int
front_prepare( fdgpu_ed25519_ctx_t * ctx, fd_front * f, unsigned long records, unsigned long keys ) {
  size_t ns = ctx->max_sig < ctx->max_txn ? ctx->max_sig : ctx->max_txn;
  if( ns > records ) ns = records;
  if( ns > ( 1UL << 24 ) ) ns = 1UL << 24;                   /* (128 ns + slack inside payload_off's 32 bits) */
  size_t pack = FD_SHRED_SLOT * ns + 2UL * FD_ARENA_SLACK;
  HIPCHK( ctx_dev_alloc( ctx, &f->d_pack, pack ), -2 );
  HIPCHK( ctx_dev_alloc( ctx, &f->d_tdesc, ns * sizeof(fdgpu_txn_desc_t) ), -2 );
  HIPCHK( ctx_dev_alloc( ctx, &f->d_code, ns ), -2 );
  HIPCHK( ctx_dev_alloc( ctx, &f->d_flag, records ), -2 );
  HIPCHK( ctx_dev_alloc( ctx, &f->d_out, records ), -2 );
  HIPCHK( ctx_dev_alloc( ctx, &f->d_root, 32UL * records ), -2 );
  HIPCHK( ctx_dev_alloc( ctx, &f->d_keys, 32UL * keys ), -2 );
  HIPCHK( hipMemsetAsync( f->d_pack, 0, pack, ctx->stream ), -2 );
  HIPCHK( hipStreamSynchronize( ctx->stream ), -2 );
  f->max = records; f->keys = keys; f->sig = ns;
  return 0;
}

/* the head and the tail that the front-ends' batches share: the slots, and the verify batch over them */
static void
front_slots( fd_front const & f, unsigned long sig_cnt, hipStream_t st ) {
  if( sig_cnt )
    hipLaunchKernelGGL( fd_shred_slot_kernel, dim3( (unsigned)( ( sig_cnt + FD_WG - 1 ) / FD_WG ) ), dim3(FD_WG), 0, st,
                        (uint4 *)f.d_pack, f.d_tdesc, (u32)sig_cnt );
}
static int
front_verify( fdgpu_ed25519_ctx_t * ctx, fd_front const & f, unsigned long sig_cnt, hipStream_t st ) {
  if( !sig_cnt ) { ctx->last_path = FDGPU_PATH_NONE; return 0; }   /* a batch without signatures */
  return launch_batch( ctx, f.d_pack, f.d_tdesc, sig_cnt, sig_cnt, f.d_code, NULL, st );
}

/* What the two host forms share.  front_arena: the arena's device address if it lies, slack included, in a
   registered region; else NULL: any other host memory, the shreds go through the staging slot, one every
   FD_SHRED_STRIDE bytes, and *most comes down to those the slot holds.  front_stage: a chunk of n staged shreds,
   zero slack behind them, up to the slot's device arena, which *da and *dsz then name. */
static int
front_arena( fdgpu_ed25519_ctx_t const * ctx, unsigned char const * arena, unsigned long arena_sz, unsigned char ** d_arena,
             unsigned long * most ) {
  if( ( *d_arena = region_dev( arena, arena_sz + FD_ARENA_SLACK ) ) ) return 0;
  if( *most > ctx->max_payload / FD_SHRED_STRIDE ) *most = ctx->max_payload / FD_SHRED_STRIDE;
  return sync_ctx( ctx, 1 );
}
static int
front_stage( fd_slot & sl, unsigned long n, unsigned char ** da, unsigned long * dsz, hipStream_t st ) {
  *dsz = FD_SHRED_STRIDE * n;
  memset( sl.h_payload + *dsz, 0, FD_ARENA_SLACK );
  HIPCHK( hipMemcpyAsync( sl.d_payload, sl.h_payload, *dsz + FD_ARENA_SLACK, hipMemcpyHostToDevice, st ), -2 );
  *da = sl.d_payload;
  return 0;
}

extern "C" int
fdgpu_ed25519_shreds_prepare( fdgpu_ed25519_ctx_t * ctx, unsigned long max_shreds, unsigned long max_keys ) {
  FRONT_CTX( ctx );
  if( !max_shreds || max_shreds >= ( 1UL << 31 ) || !max_keys || max_keys > (unsigned long)FD_SHRED_NO_SIG ) {
    fd_err = "fdgpu_ed25519_shreds_prepare: bad size"; return -1;
  }
  if( max_shreds <= ctx->sh.max && max_keys <= ctx->sh.keys ) return 0;
  HIPCHK( hipSetDevice( ctx->device ), -2 );
  if( max_shreds < ctx->sh.max  ) max_shreds = ctx->sh.max;
  if( max_keys   < ctx->sh.keys ) max_keys   = ctx->sh.keys;
  if( front_release( ctx, &ctx->sh ) ) return -2;
  ctx_dev_free( ctx, &ctx->d_sh_desc );
  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_sh_desc, max_shreds * sizeof(fdgpu_shred_desc_t) ), -2 );
  return front_prepare( ctx, &ctx->sh, max_shreds, max_keys );
}

/* the kernels of one batch of shreds on st: the slots, the roots, the batch over the slots, the codes */
static int
shreds_launch( fdgpu_ed25519_ctx_t * ctx, unsigned char const * d_arena, unsigned long arena_sz,
               fdgpu_shred_desc_t const * d_desc, unsigned long cnt, unsigned long sig_cnt, unsigned char const * d_keys,
               unsigned long key_cnt, i8 * d_out, unsigned char * d_root, hipStream_t st ) {
  fd_front const & f = ctx->sh;
  unsigned nb = (unsigned)( ( cnt + FD_WG - 1 ) / FD_WG );
  front_slots( f, sig_cnt, st );
  hipLaunchKernelGGL( fd_shred_root_kernel, dim3(nb), dim3(FD_WG), 0, st, d_arena, arena_sz, d_desc, (u32)cnt, (u32)sig_cnt,
                      (uint4 const *)d_keys, (u32)key_cnt, (uint4 *)f.d_pack, f.d_tdesc, f.d_flag, (uint4 *)d_root );
  HIPCHK( hipGetLastError(), -3 );
  int rc = front_verify( ctx, f, sig_cnt, st );
  if( rc ) return rc;
  hipLaunchKernelGGL( fd_shred_flag_kernel, dim3(nb), dim3(FD_WG), 0, st, d_desc, (u32)cnt, (i8 const *)f.d_flag,
                      (i8 const *)f.d_code, d_out );
  HIPCHK( hipGetLastError(), -3 );
  return 0;
}

extern "C" int
fdgpu_ed25519_verify_shreds_device( fdgpu_ed25519_ctx_t * ctx, unsigned char const * d_arena, unsigned long arena_sz,
                                    fdgpu_shred_desc_t const * d_desc, unsigned long cnt, unsigned long sig_cnt,
                                    unsigned char const * d_keys, unsigned long key_cnt, signed char * d_out,
                                    unsigned char * d_root, void * stream ) {
  FRONT_CTX( ctx ); FRONT_PREPARED( ctx->sh.max, "fdgpu_ed25519_shreds_prepare" );
  if( cnt > ctx->sh.max || sig_cnt > ctx->sh.sig || key_cnt > ctx->sh.keys ) { fd_err = "batch larger than prepared"; return -1; }
  if( !cnt ) return 0;
  if( !d_arena || !d_desc || !d_out || ( key_cnt && !d_keys ) ) { fd_err = "NULL argument"; return -1; }
  if( ( (uintptr_t)d_keys | (uintptr_t)d_root ) & 15UL ) { fd_err = "d_keys and d_root are 16-byte aligned"; return -1; }
  HIPCHK( hipSetDevice( ctx->device ), -2 );
  return shreds_launch( ctx, d_arena, arena_sz, d_desc, cnt, sig_cnt, d_keys, key_cnt, (i8 *)d_out, d_root,
                        stream ? (hipStream_t)stream : ctx->stream );
}

extern "C" int
fdgpu_ed25519_verify_shreds_host( fdgpu_ed25519_ctx_t * ctx, unsigned char const * arena, unsigned long arena_sz,
                                  fdgpu_shred_desc_t const * desc, unsigned long cnt, unsigned char const * keys,
                                  unsigned long key_cnt, signed char * out, unsigned char * root ) {
  FRONT_CTX( ctx ); FRONT_PREPARED( ctx->sh.max, "fdgpu_ed25519_shreds_prepare" );
  fd_front const & f = ctx->sh;
  if( key_cnt > f.keys ) { fd_err = "more keys than prepared"; return -1; }
  if( !cnt ) return 0;
  if( !arena || !desc || !out || ( key_cnt && !keys ) ) { fd_err = "NULL argument"; return -1; }
  int rc;
  unsigned char * d_arena;
  unsigned long most = f.max;
  if( ( rc = front_arena( ctx, arena, arena_sz, &d_arena, &most ) ) ) return rc;
  if( !most ) { fd_err = "the staging slot holds no shred"; return -1; }
  if( ( rc = sync_begin( ctx ) ) ) return rc;
  hipStream_t st = ctx->stream;
  fd_slot & sl = ctx->slot[0];
  if( key_cnt ) HIPCHK( hipMemcpyAsync( f.d_keys, keys, 32UL * key_cnt, hipMemcpyHostToDevice, st ), -2 );
  std::vector<fdgpu_shred_desc_t> tmp( most < cnt ? most : cnt );
  for( unsigned long done=0UL; done<cnt; ) {
    /* the chunk: records up to the prepared count, signatures -- numbered here, in order -- up to the slots */
    unsigned long n = 0UL, nsig = 0UL;
    while( done + n < cnt && n < most ) {
      fdgpu_shred_desc_t d = desc[ done + n ];
      if( d.key_idx != FD_SHRED_NO_SIG ) {
        if( nsig == f.sig ) break;
        d.sig_idx = (unsigned int)nsig++;
      }
      if( !d_arena ) {
        if( (unsigned long)d.off + (unsigned long)d.sz > arena_sz ) { d.off = 0xFFFFFFFFU; d.sz = 0xFFFFU; }   /* stays bad */
        else {
          unsigned short sz = d.sz < 1228U ? d.sz : (unsigned short)1228U;
          memcpy( sl.h_payload + FD_SHRED_STRIDE * n, arena + d.off, sz );
          d.off = (unsigned int)( FD_SHRED_STRIDE * n ); d.sz = sz;
        }
      }
      tmp[ n++ ] = d;
    }
    unsigned char * da = d_arena; unsigned long dsz = arena_sz;
    if( !d_arena && ( rc = front_stage( sl, n, &da, &dsz, st ) ) ) return rc;
    HIPCHK( hipMemcpyAsync( ctx->d_sh_desc, tmp.data(), n * sizeof(fdgpu_shred_desc_t), hipMemcpyHostToDevice, st ), -2 );
    if( ( rc = shreds_launch( ctx, da, dsz, ctx->d_sh_desc, n, nsig, f.d_keys, key_cnt, f.d_out, root ? f.d_root : NULL, st ) ) ) return rc;
    HIPCHK( hipMemcpyAsync( out + done, f.d_out, n, hipMemcpyDeviceToHost, st ), -2 );
    if( root ) HIPCHK( hipMemcpyAsync( root + 32UL * done, f.d_root, 32UL * n, hipMemcpyDeviceToHost, st ), -2 );
    if( stream_wait( ctx, st, 1 ) ) return -2;
    done += n;
  }
  return 0;
}

/* ---- FEC sets ----------------------------------------------- */

extern "C" int
fdgpu_ed25519_fec_prepare( fdgpu_ed25519_ctx_t * ctx, unsigned long max_sets, unsigned long max_members,
                           unsigned long max_keys ) {
  FRONT_CTX( ctx );
  if( !max_sets || max_sets >= ( 1UL << 31 ) || !max_members || max_members >= ( 1UL << 31 ) ||
      !max_keys || max_keys > (unsigned long)FD_SHRED_NO_SIG ) {
    fd_err = "fdgpu_ed25519_fec_prepare: bad size"; return -1;
  }
  if( max_sets <= ctx->fc.max && max_members <= ctx->fc_members && max_keys <= ctx->fc.keys ) return 0;
  HIPCHK( hipSetDevice( ctx->device ), -2 );
  if( max_sets    < ctx->fc.max     ) max_sets    = ctx->fc.max;
  if( max_members < ctx->fc_members ) max_members = ctx->fc_members;
  if( max_keys    < ctx->fc.keys    ) max_keys    = ctx->fc.keys;
  if( front_release( ctx, &ctx->fc ) ) return -2;
  ctx->fc_members = 0UL;
  ctx_dev_free( ctx, &ctx->d_fc_desc ); ctx_dev_free( ctx, &ctx->d_fc_member ); ctx_dev_free( ctx, &ctx->d_fc_expect );
  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_fc_desc, max_sets * sizeof(fdgpu_fec_desc_t) ), -2 );
  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_fc_member, max_members * sizeof(fdgpu_fec_member_t) ), -2 );
  HIPCHK( ctx_dev_alloc( ctx, &ctx->d_fc_expect, 32UL * max_sets ), -2 );
  int cus = 0;
  HIPCHK( hipDeviceGetAttribute( &cus, hipDeviceAttributeMultiprocessorCount, ctx->device ), -2 );
  ctx->fc_all = 4UL * (unsigned long)( cus > 0 ? cus : 1 );
  ctx->fc_members = max_members;
  return front_prepare( ctx, &ctx->fc, max_sets, max_keys );
}

/* the block that holds a set of most leaves: whole wavefronts */
static unsigned
fec_block( unsigned long most ) {
  if( most > FD_FEC_LEAF_MAX ) most = FD_FEC_LEAF_MAX;
  if( !most ) most = 1UL;
  return (unsigned)( 64UL * ( ( most + 63UL ) / 64UL ) );
}

/* the kernels of one batch of sets on st: the slots, the trees, the batch over the slots, the codes */
static int
fec_launch( fdgpu_ed25519_ctx_t * ctx, unsigned char * d_arena, unsigned long arena_sz, fdgpu_fec_desc_t const * d_desc,
            unsigned long set_cnt, fdgpu_fec_member_t const * d_member, unsigned long member_cnt, unsigned long sig_cnt,
            unsigned char const * d_keys, unsigned long key_cnt, unsigned char const * d_expect, i8 * d_out,
            unsigned char * d_root, unsigned block, hipStream_t st ) {
  fd_front const & f = ctx->fc;
  front_slots( f, sig_cnt, st );
  /* block: the lanes that hold the largest set, known on the host; 0: not known (the descriptors are the device's).  A
     good set has cnt <= member_cnt, which bounds the block.  While every block of that size is resident at once, one
     launch: lanes without a leaf cost nothing then, and a block of four waves has one on each SIMD of its CU, where
     one-wave blocks double up (measured: 0.40 against 0.47 ms at 1,024 sets of 64).  Beyond that, one launch per block
     size, each taking the sets of its size (0.63 against 0.80 ms at 4,096). */
  if( !block && set_cnt <= ctx->fc_all ) block = fec_block( member_cnt );
  unsigned lo = block ? block : 64U, hi = block ? block : fec_block( member_cnt );
  for( unsigned b=lo; b<=hi; b+=64U )
    hipLaunchKernelGGL( fd_fec_tree_kernel, dim3( (unsigned)set_cnt ), dim3(b), 4U * FD_FEC_LDS_WORDS( b ), st, d_arena, arena_sz,
                        d_desc, d_member, (u32)member_cnt, (u32)sig_cnt, (uint4 const *)d_keys, (u32)key_cnt,
                        (uint4 const *)d_expect, (uint4 *)f.d_pack, f.d_tdesc, f.d_flag, (uint4 *)d_root,
                        block ? 0U : b / 64U );
  HIPCHK( hipGetLastError(), -3 );
  int rc = front_verify( ctx, f, sig_cnt, st );
  if( rc ) return rc;
  hipLaunchKernelGGL( fd_fec_flag_kernel, dim3( (unsigned)( ( set_cnt + FD_WG - 1 ) / FD_WG ) ), dim3(FD_WG), 0, st, d_desc,
                      (u32)set_cnt, (i8 const *)f.d_flag, (i8 const *)f.d_code, d_out );
  HIPCHK( hipGetLastError(), -3 );
  return 0;
}

extern "C" int
fdgpu_ed25519_verify_fec_sets_device( fdgpu_ed25519_ctx_t * ctx, unsigned char * d_arena, unsigned long arena_sz,
                                      fdgpu_fec_desc_t const * d_desc, unsigned long set_cnt,
                                      fdgpu_fec_member_t const * d_member, unsigned long member_cnt, unsigned long sig_cnt,
                                      unsigned char const * d_keys, unsigned long key_cnt, unsigned char const * d_expect,
                                      signed char * d_out, unsigned char * d_root, void * stream ) {
  FRONT_CTX( ctx ); FRONT_PREPARED( ctx->fc.max, "fdgpu_ed25519_fec_prepare" );
  if( set_cnt > ctx->fc.max || member_cnt > ctx->fc_members || sig_cnt > ctx->fc.sig || key_cnt > ctx->fc.keys ) {
    fd_err = "batch larger than prepared"; return -1;
  }
  if( !set_cnt ) return 0;
  if( !d_arena || !d_desc || !d_out || ( member_cnt && !d_member ) || ( key_cnt && !d_keys ) ) { fd_err = "NULL argument"; return -1; }
  if( ( (uintptr_t)d_keys | (uintptr_t)d_root | (uintptr_t)d_expect ) & 15UL ) {
    fd_err = "d_keys, d_root and d_expect are 16-byte aligned"; return -1;
  }
  HIPCHK( hipSetDevice( ctx->device ), -2 );
  return fec_launch( ctx, d_arena, arena_sz, d_desc, set_cnt, d_member, member_cnt, sig_cnt, d_keys, key_cnt, d_expect,
                     (i8 *)d_out, d_root, 0U, stream ? (hipStream_t)stream : ctx->stream );
}

/* leaves of a set whose members the host form uploads: 0 for a set that is bad whatever its members are */
static unsigned long
fec_need( fdgpu_fec_desc_t const & d, unsigned long member_cnt ) {
  if( !d.cnt || d.cnt > FD_FEC_LEAF_MAX || (unsigned long)d.member0 + (unsigned long)d.cnt > member_cnt ) return 0UL;
  return (unsigned long)d.cnt;
}

extern "C" int
fdgpu_ed25519_verify_fec_sets_host( fdgpu_ed25519_ctx_t * ctx, unsigned char * arena, unsigned long arena_sz,
                                    fdgpu_fec_desc_t const * desc, unsigned long set_cnt,
                                    fdgpu_fec_member_t const * member, unsigned long member_cnt,
                                    unsigned char const * keys, unsigned long key_cnt, unsigned char const * expect,
                                    signed char * out, unsigned char * root ) {
  FRONT_CTX( ctx ); FRONT_PREPARED( ctx->fc.max, "fdgpu_ed25519_fec_prepare" );
  fd_front const & f = ctx->fc;
  if( key_cnt > f.keys ) { fd_err = "more keys than prepared"; return -1; }
  if( !set_cnt ) return 0;
  if( !arena || !desc || !out || ( member_cnt && !member ) || ( key_cnt && !keys ) ) { fd_err = "NULL argument"; return -1; }
  int rc;
  unsigned char * d_arena;
  unsigned long most = ctx->fc_members;                       /* members, each with its shred, of a chunk */
  if( ( rc = front_arena( ctx, arena, arena_sz, &d_arena, &most ) ) ) return rc;
  for( unsigned long s=0UL; s<set_cnt; s++ ) {
    if( ( desc[s].flags & FD_FEC_CHECK_ROOT ) && !expect ) { fd_err = "FDGPU_FEC_CHECK_ROOT without expect"; return -1; }
    if( fec_need( desc[s], member_cnt ) > most ) { fd_err = "a set holds more members than a batch may"; return -1; }
  }
  if( ( rc = sync_begin( ctx ) ) ) return rc;
  hipStream_t st = ctx->stream;
  fd_slot & sl = ctx->slot[0];
  if( key_cnt ) HIPCHK( hipMemcpyAsync( f.d_keys, keys, 32UL * key_cnt, hipMemcpyHostToDevice, st ), -2 );
  std::vector<fdgpu_fec_desc_t>   td;
  std::vector<fdgpu_fec_member_t> tm;
  std::vector<unsigned int>       from;                       /* staged: where member k's shred came from */
  std::vector<i8>                 fl;
  for( unsigned long done=0UL; done<set_cnt; ) {
    /* the chunk: whole sets up to the prepared counts, signatures -- numbered here, in order -- up to the slots */
    unsigned long n = 0UL, nm = 0UL, nsig = 0UL, big = 0UL;
    int any_fill = 0;
    td.clear(); tm.clear(); from.clear();
    while( done + n < set_cnt && n < f.max ) {
      fdgpu_fec_desc_t d = desc[ done + n ];
      unsigned long need = fec_need( d, member_cnt );
      if( nm + need > most ) break;
      if( d.key_idx != FD_SHRED_NO_SIG ) {
        if( nsig == f.sig ) break;
        d.sig_idx = (unsigned int)nsig++;
      }
      if( !need ) d.member0 = 0xFFFFFFFFU;                     /* stays bad */
      else {
        for( unsigned long j=0UL; j<need; j++ ) {
          fdgpu_fec_member_t m = member[ (unsigned long)d.member0 + j ];
          any_fill |= (int)( m.flags & FD_FEC_FILL );
          if( !d_arena ) {
            unsigned long k = nm + j;
            from.push_back( m.off );
            int bad = fd_fec_range_bad( m.off, arena_sz, 0, 0U );
            if( !bad ) bad = fd_fec_range_bad( m.off, arena_sz, 1, arena[ (unsigned long)m.off + 0x40UL ] );
            if( bad ) m.off = 0xFFFFFFFFU;                     /* stays bad */
            else {
              unsigned long sz = fd_shred_is_code( arena[ (unsigned long)m.off + 0x40UL ] & 0xf0U ) ? FD_SHRED_CODE_SZ : FD_SHRED_DATA_SZ;
              memcpy( sl.h_payload + FD_SHRED_STRIDE * k, arena + m.off, sz );
              m.off = (unsigned int)( FD_SHRED_STRIDE * k );
            }
          }
          tm.push_back( m );
        }
        d.member0 = (unsigned int)nm;
        nm += need;
        if( need > big ) big = need;
      }
      td.push_back( d );
      n++;
    }
    if( !n ) { fd_err = "fdgpu_ed25519_verify_fec_sets_host: no signature slot"; return -1; }
    unsigned char * da = d_arena; unsigned long dsz = arena_sz;
    if( !d_arena && ( rc = front_stage( sl, nm, &da, &dsz, st ) ) ) return rc;
    HIPCHK( hipMemcpyAsync( ctx->d_fc_desc, td.data(), n * sizeof(fdgpu_fec_desc_t), hipMemcpyHostToDevice, st ), -2 );
    if( nm ) HIPCHK( hipMemcpyAsync( ctx->d_fc_member, tm.data(), nm * sizeof(fdgpu_fec_member_t), hipMemcpyHostToDevice, st ), -2 );
    if( expect ) HIPCHK( hipMemcpyAsync( ctx->d_fc_expect, expect + 32UL * done, 32UL * n, hipMemcpyHostToDevice, st ), -2 );
    if( ( rc = fec_launch( ctx, da, dsz, ctx->d_fc_desc, n, ctx->d_fc_member, nm, nsig, f.d_keys, key_cnt,
                           expect ? ctx->d_fc_expect : NULL, f.d_out, root ? f.d_root : NULL, fec_block( big ), st ) ) ) return rc;
    HIPCHK( hipMemcpyAsync( out + done, f.d_out, n, hipMemcpyDeviceToHost, st ), -2 );
    if( root ) HIPCHK( hipMemcpyAsync( root + 32UL * done, f.d_root, 32UL * n, hipMemcpyDeviceToHost, st ), -2 );
    int back = !d_arena && any_fill && nm;
    if( back ) {
      fl.resize( n );
      HIPCHK( hipMemcpyAsync( fl.data(), f.d_flag, n, hipMemcpyDeviceToHost, st ), -2 );
      HIPCHK( hipMemcpyAsync( sl.h_payload, sl.d_payload, dsz, hipMemcpyDeviceToHost, st ), -2 );
    }
    if( stream_wait( ctx, st, 1 ) ) return -2;
    if( back ) {
      /* the proofs the GPU wrote into the staged shreds of sets that passed, to where the shreds came from */
      for( unsigned long s=0UL; s<n; s++ ) {
        if( fl[s] || td[s].member0 == 0xFFFFFFFFU ) continue;
        unsigned long D = fd_fec_depth( td[s].cnt );
        for( unsigned long j=0UL; j<td[s].cnt; j++ ) {
          unsigned long k = (unsigned long)td[s].member0 + j;
          if( !( tm[k].flags & FD_FEC_FILL ) ) continue;
          unsigned char const * b = sl.h_payload + FD_SHRED_STRIDE * k;
          unsigned int w[ FD_SHRED_FIELD_WORDS ];
          memcpy( w, b + 64, sizeof(w) );
          fd_shred_fields_t f; fd_shred_info_t in;
          fd_shred_fields( w, &f );
          if( fd_shred_classify( &f, FD_SHRED_CODE_SZ, FD_SHRED_STRICT_LEAF, &in ) ) continue;   /* (a set that passed: it classifies) */
          memcpy( arena + from[k] + in.moff, b + in.moff, FD_SHRED_NODE_SZ * D );
        }
      }
    }
    done += n;
  }
  return 0;
}

/* ---- batch SHA-256 ---------------------------------------------------- */

extern "C" int
fdgpu_sha256_batch_device( unsigned char const * d_data, unsigned long const * d_off, unsigned int const * d_sz,
                           unsigned long cnt, unsigned char * d_hash, void * stream ) {
  if( !cnt ) return 0;
  if( cnt >= (1UL<<31) ) { fd_err = "batch too large"; return -1; }
  unsigned g = (unsigned)( (cnt + FD_WG - 1) / FD_WG );
  hipLaunchKernelGGL( fd_sha256_batch_kernel, dim3(g), dim3(FD_WG), 0, (hipStream_t)stream, d_data, d_off, d_sz,
                      (u32)cnt, (uint4 *)d_hash );
  HIPCHK( hipGetLastError(), -3 );
  return 0;
}

/* The host form of a hash batch: digests of HASH_SZ bytes by batch_device, which reads up to SLACK bytes past a
   message; a message of SZ_LIM bytes or more is refused like one that leaves the buffer (1 << 32: none is). */
template< unsigned long HASH_SZ, size_t SLACK, unsigned long SZ_LIM, class F > static int
hash_batch_host( int device, unsigned char const * data, unsigned long data_sz, unsigned long const * off,
                 unsigned int const * sz, unsigned long cnt, unsigned char * hash, F batch_device ) {
  if( !cnt ) return 0;
  for( unsigned long t=0; t<cnt; t++ )
    if( off[t] > data_sz || sz[t] > data_sz - off[t] || sz[t] >= SZ_LIM ) { fd_err = "message out of buffer"; return -1; }
  HIPCHK( hipSetDevice( device ), -2 );
  unsigned char * d_data = NULL, * d_hash = NULL; unsigned long * d_off = NULL; unsigned int * d_sz = NULL;
  int rc = -2;
  if( hipMalloc( (void **)&d_data, data_sz + SLACK ) != hipSuccess ||
      hipMalloc( (void **)&d_off, cnt * sizeof(unsigned long) ) != hipSuccess ||
      hipMalloc( (void **)&d_sz, cnt * sizeof(unsigned int) ) != hipSuccess ||
      hipMalloc( (void **)&d_hash, cnt * HASH_SZ ) != hipSuccess ) { fd_err = "hipMalloc failed"; goto done; }
  if( hipMemset( d_data + data_sz, 0, SLACK ) != hipSuccess ||
      ( data_sz && hipMemcpy( d_data, data, data_sz, hipMemcpyHostToDevice ) != hipSuccess ) ||
      hipMemcpy( d_off, off, cnt * sizeof(unsigned long), hipMemcpyHostToDevice ) != hipSuccess ||
      hipMemcpy( d_sz, sz, cnt * sizeof(unsigned int), hipMemcpyHostToDevice ) != hipSuccess ) { fd_err = "upload failed"; goto done; }
  rc = batch_device( d_data, d_off, d_sz, cnt, d_hash, NULL );
  if( !rc && hipMemcpy( hash, d_hash, cnt * HASH_SZ, hipMemcpyDeviceToHost ) != hipSuccess ) { fd_err = "download failed"; rc = -2; }
done:
  hipFree( d_data ); hipFree( d_off ); hipFree( d_sz ); hipFree( d_hash );
  return rc;
}

extern "C" int
fdgpu_sha256_batch_host( int device, unsigned char const * data, unsigned long data_sz, unsigned long const * off,
                         unsigned int const * sz, unsigned long cnt, unsigned char * hash ) {
  /* (fd_sha256_bytes reads up to 67 bytes past a message) */
  return hash_batch_host< 32UL, 128, 1UL << 29 >( device, data, data_sz, off, sz, cnt, hash, fdgpu_sha256_batch_device );
}

/* ---- batch SHA-512 ---------------------------------------------------- */

extern "C" int
fdgpu_sha512_batch_device( unsigned char const * d_data, unsigned long const * d_off, unsigned int const * d_sz,
                           unsigned long cnt, unsigned char * d_hash, void * stream ) {
  if( !cnt ) return 0;
  if( cnt >= (1UL<<31) ) { fd_err = "batch too large"; return -1; }
  unsigned g = (unsigned)( (cnt + FD_WG - 1) / FD_WG );
  hipLaunchKernelGGL( fd_sha512_batch_kernel, dim3(g), dim3(FD_WG), 0, (hipStream_t)stream, d_data, d_off, d_sz,
                      (u32)cnt, (uint4 *)d_hash );
  HIPCHK( hipGetLastError(), -3 );
  return 0;
}

extern "C" int
fdgpu_sha512_batch_host( int device, unsigned char const * data, unsigned long data_sz, unsigned long const * off,
                         unsigned int const * sz, unsigned long cnt, unsigned char * hash ) {
  /* (fd_sha512_bytes reads past the last block) */
  return hash_batch_host< 64UL, 256, 1UL << 32 >( device, data, data_sz, off, sz, cnt, hash, fdgpu_sha512_batch_device );
}

/* ---- raw-payload batches (device fd_txn_parse + verify) ------------- */

extern "C" int
fdgpu_txn_parse_device( unsigned char const * d_payload, fdgpu_txn_raw_t const * d_raw, unsigned long txn_cnt,
                        unsigned char * d_img, unsigned long img_stride, unsigned short * d_fp, void * stream ) {
  if( !txn_cnt ) return 0;
  if( txn_cnt >= (1UL<<31) || ( d_img && ( img_stride < 852UL || img_stride > 0xffffffffUL ) ) ) { fd_err = "bad arguments"; return -1; }
  unsigned g = (unsigned)( (txn_cnt + FD_WG - 1) / FD_WG );
  hipLaunchKernelGGL( fd_parse_kernel, dim3(g), dim3(FD_WG), 0, (hipStream_t)stream, d_payload, d_raw, (u32)txn_cnt,
                      (fdgpu_txn_desc_t *)NULL, (unsigned char *)NULL, d_img, (u32)img_stride, d_fp, fd_seeds{}, (u64 *)NULL,
                      (unsigned char const *)NULL , (u32 *)NULL, 0u, (u32 *)NULL, (unsigned long *)NULL);
  HIPCHK( hipGetLastError(), -3 );
  return 0;
}

/* fused = 1 (the async pipeline): the parse kernel also writes the signature map (no fd_expand_kernel)
   and the batch's start stamp, and the reduce is left to the caller's fd_finish_kernel */
static int launch_raw( fdgpu_ed25519_ctx_t * ctx, unsigned char const * d_payload, fdgpu_txn_raw_t const * d_raw,
                       unsigned long txn_cnt, unsigned long sig_cnt, i8 * d_txn_out, unsigned char * d_img,
                       unsigned long img_stride, unsigned short * d_fp, hipStream_t st, u64 * d_dtag = NULL,
                       unsigned char const * d_ovr = NULL, int fused = 0, unsigned long * stamp = NULL ) {
  if( !txn_cnt ) return 0;
  unsigned g = (unsigned)( (txn_cnt + FD_WG - 1) / FD_WG );
  fd_seeds ds;
  memset( &ds, 0, sizeof(ds) );
  ds.seed[0] = (u64)ctx->dedup_seed;
  int nseed = __atomic_load_n( &ctx->dedup_nseed, __ATOMIC_ACQUIRE );
  if( nseed ) {
    for( int i=0; i<16; i++ ) ds.seed[i] = (u64)__atomic_load_n( &ctx->dedup_seeds[i], __ATOMIC_RELAXED );
    ds.nseed = (u32)nseed;
  }
  hipLaunchKernelGGL( fd_parse_kernel, dim3(g), dim3(FD_WG), 0, st, d_payload, d_raw, (u32)txn_cnt,
                      ctx->d_rdesc, ctx->d_pflag, d_img, (u32)img_stride, d_fp, ds, d_dtag, d_ovr,
                      fused ? ctx->d_map : (u32 *)NULL, (u32)sig_cnt, fused ? slow_word( ctx, FD_SW_SLOW ) : (u32 *)NULL,
                      stamp );
  HIPCHK( hipGetLastError(), -3 );
  return launch_batch( ctx, d_payload, ctx->d_rdesc, txn_cnt, sig_cnt, d_txn_out, NULL, st, ctx->d_pflag,
                       fused ? 3 : 0 );
}

extern "C" int
fdgpu_ed25519_verify_raw_device( fdgpu_ed25519_ctx_t * ctx, unsigned char const * d_payload, fdgpu_txn_raw_t const * d_raw,
                                 unsigned long txn_cnt, unsigned long sig_cnt, signed char * d_txn_out,
                                 unsigned char * d_img, unsigned long img_stride, unsigned short * d_fp, void * stream ) {
  if( !ctx ) { fd_err = "NULL ctx"; return -1; }
  if( txn_cnt > ctx->max_txn || sig_cnt > ctx->max_sig ) { fd_err = "batch larger than ctx"; return -1; }
  if( d_img && ( img_stride < 852UL || img_stride > 0xffffffffUL ) ) { fd_err = "img_stride < FD_TXN_MAX_SZ"; return -1; }
  HIPCHK( hipSetDevice( ctx->device ), -2 );
  return launch_raw( ctx, d_payload, d_raw, txn_cnt, sig_cnt, (i8 *)d_txn_out, d_img, img_stride, d_fp,
                     stream ? (hipStream_t)stream : ctx->stream );
}

/* signature lanes of a raw payload: its first byte (the parsed signature_cnt, fd_txn_parse.c:86),
   0 where that cannot be a count */
static inline unsigned raw_lanes( unsigned char const * payload, unsigned long payload_sz ) {
  unsigned b0 = payload_sz ? payload[0] : 0u;
  return ( b0 >= 1u && b0 <= 16u ) ? b0 : 0u;
}

/* host side of the raw path: each payload's signature lanes and their prefix */
static int stage_raw( unsigned char const * payload, unsigned long payload_bytes, fdgpu_txn_raw_t * raw,
                      unsigned long txn_cnt, unsigned long * sig_total ) {
  unsigned long s = 0;
  for( unsigned long i=0; i<txn_cnt; i++ ) {
    if( (unsigned long)raw[i].payload_off + raw[i].payload_sz > payload_bytes ) { fd_err = "payload out of arena"; return -1; }
    raw[i].sig_lanes = (unsigned char)raw_lanes( payload + raw[i].payload_off, raw[i].payload_sz );
    raw[i].sig_base  = (unsigned)s;
    s += raw[i].sig_lanes;
  }
  *sig_total = s;
  return 0;
}

extern "C" int
fdgpu_ed25519_verify_raw_host( fdgpu_ed25519_ctx_t * ctx, unsigned char const * payload, unsigned long payload_bytes,
                               fdgpu_txn_raw_t * raw, unsigned long txn_cnt, signed char * txn_out,
                               unsigned char * img, unsigned long img_stride, unsigned short * fp ) {
  int rc = sync_ctx( ctx, 0 );
  if( rc ) return rc;
  unsigned long nsig;
  if( stage_raw( payload, payload_bytes, raw, txn_cnt, &nsig ) ) return -1;
  if( txn_cnt > ctx->max_txn || nsig > ctx->max_sig || payload_bytes > ctx->max_payload ) { fd_err = "batch larger than ctx"; return -1; }
  if( img && img_stride < 852UL ) { fd_err = "img_stride < FD_TXN_MAX_SZ"; return -1; }
  if( !txn_cnt ) return 0;
  if( ( rc = sync_begin( ctx ) ) ) return rc;
  fd_slot & sl = ctx->slot[0];
  memcpy( sl.h_payload, payload, payload_bytes );
  memset( sl.h_payload + payload_bytes, 0, FD_ARENA_SLACK );
  memcpy( sl.h_desc, raw, txn_cnt * sizeof(fdgpu_txn_raw_t) );
  hipStream_t st = ctx->stream;
  unsigned char * d_img = NULL; unsigned short * d_fp = NULL;
  if( img ) HIPCHK( hipMallocAsync( (void **)&d_img, txn_cnt * img_stride, st ), -2 );
  if( fp  ) HIPCHK( hipMallocAsync( (void **)&d_fp,  txn_cnt * sizeof(unsigned short), st ), -2 );
  HIPCHK( hipMemcpyAsync( sl.d_payload, sl.h_payload, payload_bytes + FD_ARENA_SLACK, hipMemcpyHostToDevice, st ), -2 );
  HIPCHK( hipMemcpyAsync( sl.d_desc, sl.h_desc, txn_cnt * sizeof(fdgpu_txn_raw_t), hipMemcpyHostToDevice, st ), -2 );
  if( ( rc = launch_raw( ctx, sl.d_payload, (fdgpu_txn_raw_t const *)sl.d_desc, txn_cnt, nsig, sl.d_txn_out, d_img,
                         img_stride, d_fp, st ) ) ) return rc;
  if( img ) { HIPCHK( hipMemcpyAsync( img, d_img, txn_cnt * img_stride, hipMemcpyDeviceToHost, st ), -2 ); HIPCHK( hipFreeAsync( d_img, st ), -2 ); }
  if( fp  ) { HIPCHK( hipMemcpyAsync( fp, d_fp, txn_cnt * sizeof(unsigned short), hipMemcpyDeviceToHost, st ), -2 ); HIPCHK( hipFreeAsync( d_fp, st ), -2 ); }
  return sync_finish( ctx, txn_cnt, txn_out, NULL, 0UL, img || fp );
}

/* ---- async submit / poll ------------------------------------------ */

/* One stream per context: upload, kernels and download of a slot are
   in stream order.  (A separate copy stream with cross-stream event
   waits deadlocked once several contexts' streams were multiplexed onto
   the device's few hardware queues -- a waiter's barrier packet can sit
   ahead of the work it waits for in a shared queue.  Overlap of one
   context's upload with another's kernels comes from running several
   contexts, one per verify tile.) */
/* launch the gather of slot sl's records not yet gathered (mode 3) on the
   context's gather stream; returns how many, or < 0 */
/* GPU pauses, process-wide (fdgpu_debug_gather_pauses): the first FD_PAUSE_LOG timed gathers that waited over
   250 us on the GPU after their runtime call -- host time of the call and the wait, ns */
#define FD_PAUSE_LOG 512
static unsigned long             g_pause[ FD_PAUSE_LOG ][ 2 ];
static std::atomic<unsigned long> g_pause_n{ 0 };

/* account the timed gathers whose count has been reached */
static void gather_times( fdgpu_ed25519_ctx_t * ctx, unsigned long gathered ) {
  while( ctx->gt_head < ctx->gt_tail && ctx->gt[ ctx->gt_head % FD_NGT ].target <= gathered ) {
    unsigned long i = ctx->gt_head % FD_NGT;
    unsigned long const volatile * w = (unsigned long const volatile *)( ctx->h_gtime + 2*i );
    if( ctx->gclk_ok && w[0] && w[1] >= w[0] ) {
      double st = (double)w[0] * 10.0 - ctx->gclk_off_ns - (double)ctx->gt[i].t_launch;
      unsigned long sd = st > 0. ? (unsigned long)st : 0UL, rn = ( w[1] - w[0] ) * 10UL;
      unsigned long ti = __atomic_load_n( &ctx->gt[i].t_issue, __ATOMIC_ACQUIRE );
      double si = ti ? (double)w[0] * 10.0 - ctx->gclk_off_ns - (double)ti : 0.;
      unsigned long sdi = si > 0. ? (unsigned long)si : 0UL;
      ctx->gs_issue_sum += sdi;
      if( sdi > ctx->gs_issue_max ) ctx->gs_issue_max = sdi;
      ctx->gs_issue_slow += sdi > 250000UL;
      if( sdi > 250000UL ) {
        unsigned long e = g_pause_n.fetch_add( 1UL, std::memory_order_relaxed );
        if( e < FD_PAUSE_LOG ) { g_pause[e][0] = ti; g_pause[e][1] = sdi; }
      }
      ctx->gs_n++; ctx->gs_start_sum += sd; ctx->gs_run_sum += rn;
      if( sd > ctx->gs_start_max ) ctx->gs_start_max = sd;
      if( rn > ctx->gs_run_max ) ctx->gs_run_max = rn;
    }
    ctx->gt_head++;
  }
}

/* the gather stream and its timing ring (on first use, or by fdgpu_ed25519_prepare) */
static int gather_init( fdgpu_ed25519_ctx_t * ctx ) {
  if( !ctx->h_gtime )
    HIPCHK( ctx_pin_alloc( ctx, &ctx->h_gtime, ( FD_NGT + 1 ) * 2 * sizeof(unsigned long), &ctx->d_gtime ), -2 );
  if( !ctx->gstream ) {
    /* the copies bound how long a frag stays exposed to a lapping producer: the highest stream
       priority, so the dispatcher starts them ahead of queued verify work as CU slots free up */
    int lo = 0, hi = 0;
    HIPCHK( hipDeviceGetStreamPriorityRange( &lo, &hi ), -2 );
    HIPCHK( hipStreamCreateWithPriority( &ctx->gstream, hipStreamNonBlocking, hi ), -2 );
    HIPCHK( hipEventCreateWithFlags( &ctx->gev, hipEventDisableTiming ), -2 );
  }
  return 0;
}

/* A gather's launch, split in two: gather_prep does the host bookkeeping (counts, timing ring) on the
   caller's thread, gather_issue the runtime call -- on the caller's thread, or on the context's launch
   thread (fdgpu_ed25519_set_launcher) with the arguments prep captured */
struct fd_gargs {
  struct fd_gather const * g;
  u32                      n;
  unsigned char *          d_payload;
  unsigned char *          wb;       /* the records' write-back base (NULL: none) */
  unsigned char *          ovr;
  unsigned long            target;
  unsigned long *          gt;
  long                     gti;      /* its timing-ring entry (the issue time goes there), -1: untimed */
};

/* the gather of slot sl's records not yet gathered: 0 if none, else how many (a filled) or < 0 */
static long gather_prep( fdgpu_ed25519_ctx_t * ctx, fd_slot & sl, fd_gargs * a ) {
  unsigned long n = sl.txn_cnt - sl.gathered;
  if( !n ) return 0;
  if( gather_init( ctx ) ) return -2;
  unsigned long target = ctx->g_launched + n;
  /* time this gather if a ring entry is free (the ring is drained as gathers complete) */
  unsigned long * gt = NULL;
  gather_times( ctx, fdgpu_ed25519_gathered( ctx ) );
  if( ctx->gt_tail - ctx->gt_head < FD_NGT ) {
    unsigned long i = ctx->gt_tail % FD_NGT;
    ctx->h_gtime[ 2*i ] = 0UL; ctx->h_gtime[ 2*i + 1 ] = 0UL;
    ctx->gt[i].target = target; ctx->gt[i].t_launch = fd_now_ns();
    __atomic_store_n( &ctx->gt[i].t_issue, 0UL, __ATOMIC_RELAXED );
    ctx->gt_tail++;
    gt = ctx->d_gtime + 2*i;
    ctx->last_gt = (long)i;
  } else { gt = ctx->d_gtime + 2*FD_NGT; ctx->last_gt = -1; }   /* untimed: a scratch entry */
  a->g = sl.g_dev + sl.gathered; a->n = (u32)n; a->d_payload = sl.d_payload;
  a->wb = ctx->gather_nowb == 0 && !sl.per_rec ? sl.ref_dev + sl.ref_lo : (unsigned char *)NULL;
  a->ovr = sl.d_ovr + sl.gathered; a->target = target; a->gt = gt; a->gti = ctx->last_gt;
  ctx->g_launched = target; sl.gathered = sl.txn_cnt;
  return (long)n;
}

static int gather_issue( fdgpu_ed25519_ctx_t * ctx, fd_gargs const * a ) {
  unsigned long rpb = ctx->gather_rpb == 1 ? 1UL : 4UL;
  if( a->gti >= 0 ) __atomic_store_n( &ctx->gt[ a->gti ].t_issue, fd_now_ns(), __ATOMIC_RELEASE );
  hipLaunchKernelGGL( ( rpb == 1UL ? fd_gather_kernel<1> : fd_gather_kernel<4> ), dim3( (unsigned)( ( a->n + rpb - 1UL ) / rpb ) ),
                      dim3( 64UL * rpb ), 0, ctx->gstream, a->g, a->n, a->d_payload, a->wb, a->ovr, ctx->d_gcnt,
                      (unsigned long *)( ctx->d_flag + FD_NSLOT + 1 ), a->target, a->gt );
  HIPCHK( hipGetLastError(), -2 );
  return 0;
}

/* ---- launch thread --------------------------------------------------------
   A verify tile's host loop is the paced leg's bound near its knee: at 10M frags/s a 2.8K-frag batch's ~10
   runtime calls (its last gather, the event hand-off, parse, prep, walk, slow list, finish, done, the
   completion event) take ~43 us of the tile's thread and each early copy ~10 us (profiles/r04/final5: 15.3
   and ~20 ns per frag of a 100 ns budget), during which it takes no frag and polls no verdict.  With a
   launcher the tile only fills the slot and queues one command; a thread of its own, spinning on its own
   core, makes the calls in queue order (one queue per launcher: a context's commands stay in order).  The
   slot's host state (token, in-flight list, gather counts) stays with the caller, so polling is unchanged:
   a batch is complete when fd_done_kernel's token appears.  A failed call faults the context (as a failed
   batch does) and later commands of a faulted context are dropped. */
struct fd_lcmd {
  fdgpu_ed25519_ctx_t * ctx;
  int                   kind;        /* 0: gather (g), 1: slot launch (slot, token, g if has_g) */
  int                   slot, has_g;
  unsigned long         token;
  fd_gargs              g;
};

#define FD_NCMD 512
struct fdgpu_launcher {
  fd_lcmd                    cmd[ FD_NCMD ];
  alignas(64) std::atomic<unsigned long> tail{ 0 };   /* written by the queueing thread */
  alignas(64) std::atomic<unsigned long> head{ 0 };   /* written by the launch thread */
  alignas(64) std::atomic<int>           stop{ 0 };
  int                        device, cpu;
  std::thread                th;
  unsigned long              n_cmd, busy_ns, depth_max;   /* launch thread's */
  unsigned long              max_ns, n_slow;              /* ... longest command, commands over 250 us */
  unsigned long              full_waits;                  /* queueing thread's */
};

static int slot_issue( fdgpu_ed25519_ctx_t * ctx, int i, unsigned long token, fd_gargs const * g );

static void launcher_main( fdgpu_launcher_t * L ) {
  if( L->cpu >= 0 ) {
    cpu_set_t set; CPU_ZERO( &set ); CPU_SET( L->cpu, &set );
    (void)pthread_setaffinity_np( pthread_self(), sizeof(set), &set );
  }
  (void)hipSetDevice( L->device );
  for(;;) {
    unsigned long h = L->head.load( std::memory_order_relaxed ), t = L->tail.load( std::memory_order_acquire );
    if( h == t ) {
      if( L->stop.load( std::memory_order_acquire ) ) break;
      __builtin_ia32_pause();
      continue;
    }
    if( t - h > L->depth_max ) L->depth_max = t - h;
    fd_lcmd const & c = L->cmd[ h % FD_NCMD ];
    unsigned long t0 = fd_now_ns();
    if( !__atomic_load_n( &c.ctx->fault, __ATOMIC_ACQUIRE ) ) {
      int rc;
      if( c.kind != 0 && __atomic_load_n( &c.ctx->dbg_fail_issue, __ATOMIC_ACQUIRE ) ) {   /* test hook */
        fd_err = "slot_issue: injected by fdgpu_ed25519_debug_fail_launch"; rc = -2;
      } else rc = c.kind == 0 ? gather_issue( c.ctx, &c.g ) : slot_issue( c.ctx, c.slot, c.token, c.has_g ? &c.g : NULL );
      if( rc ) {
        snprintf( c.ctx->lerr, sizeof(c.ctx->lerr), "launch thread: %s", fd_err.c_str() );
        __atomic_store_n( &c.ctx->fault, 1, __ATOMIC_RELEASE );
      }
    }
    unsigned long dt = fd_now_ns() - t0;
    L->busy_ns += dt; L->n_cmd++;
    if( dt > L->max_ns ) L->max_ns = dt;
    L->n_slow += dt > 250000UL;
    L->head.store( h + 1, std::memory_order_release );
  }
}

static void launcher_push( fdgpu_launcher_t * L, fd_lcmd const & c ) {
  unsigned long t = L->tail.load( std::memory_order_relaxed );
  if( t - L->head.load( std::memory_order_acquire ) >= FD_NCMD ) {
    L->full_waits++;
    while( t - L->head.load( std::memory_order_acquire ) >= FD_NCMD ) __builtin_ia32_pause();
  }
  L->cmd[ t % FD_NCMD ] = c;
  L->tail.store( t + 1, std::memory_order_release );
}

/* every command queued so far has been issued */
static void launcher_drain( fdgpu_launcher_t * L ) {
  unsigned long t = L->tail.load( std::memory_order_relaxed );
  while( L->head.load( std::memory_order_acquire ) < t ) __builtin_ia32_pause();
}

extern "C" fdgpu_launcher_t *
fdgpu_launcher_new( int device, int cpu ) {
  fdgpu_launcher_t * L = new fdgpu_launcher_t();
  L->device = device; L->cpu = cpu; L->n_cmd = L->busy_ns = L->depth_max = L->full_waits = L->max_ns = L->n_slow = 0UL;
  try { L->th = std::thread( launcher_main, L ); }
  catch( ... ) { delete L; fd_err = "fdgpu_launcher_new: no thread"; return NULL; }
  return L;
}

extern "C" void
fdgpu_launcher_delete( fdgpu_launcher_t * L ) {
  if( !L ) return;
  launcher_drain( L );
  L->stop.store( 1, std::memory_order_release );
  L->th.join();
  delete L;
}

extern "C" unsigned long
fdgpu_debug_gather_pauses( unsigned long * out, unsigned long n, int reset ) {
  unsigned long m = g_pause_n.load( std::memory_order_acquire );
  if( m > FD_PAUSE_LOG ) m = FD_PAUSE_LOG;
  if( m > n ) m = n;
  for( unsigned long i=0; i<m; i++ ) { out[2*i] = g_pause[i][0]; out[2*i+1] = g_pause[i][1]; }
  unsigned long tot = g_pause_n.load( std::memory_order_acquire );
  if( reset ) g_pause_n.store( 0UL, std::memory_order_release );
  return tot;
}

extern "C" void
fdgpu_launcher_stats( fdgpu_launcher_t const * L, unsigned long out[ 6 ] ) {
  out[0] = L->n_cmd; out[1] = L->busy_ns; out[2] = L->depth_max; out[3] = L->full_waits; out[4] = L->max_ns;
  out[5] = L->n_slow;
}

extern "C" int
fdgpu_ed25519_set_launcher( fdgpu_ed25519_ctx_t * ctx, fdgpu_launcher_t * L ) {
  if( !ctx ) return -1;
  if( ctx->launcher == L ) return 0;
  if( async_busy( ctx ) ) { fd_err = "fdgpu_ed25519_set_launcher: async batches pending or in flight"; return -1; }
  if( L && L->device != ctx->device ) { fd_err = "fdgpu_ed25519_set_launcher: launcher of another device"; return -1; }
  if( ctx->launcher ) launcher_drain( ctx->launcher );
  if( L && gather_init( ctx ) ) return -2;     /* the gather stream now: the launch thread only issues */
  ctx->launcher = L;
  return 0;
}

/* the gather of the filling slot's new records, on the caller's thread or queued */
static long gather_launch( fdgpu_ed25519_ctx_t * ctx, fd_slot & sl ) {
  fd_lcmd c;
  long n = gather_prep( ctx, sl, &c.g );
  if( n <= 0 ) return n;
  if( ctx->launcher ) {
    c.ctx = ctx; c.kind = 0; c.slot = -1; c.has_g = 1; c.token = 0UL;
    launcher_push( ctx->launcher, c );
    return n;
  }
  if( gather_issue( ctx, &c.g ) ) return -2;
  return n;
}

/* the runtime calls of slot i's batch, in stream order (token: the value fd_done_kernel stores; g: the
   batch's last gather, if any) */
static int slot_issue( fdgpu_ed25519_ctx_t * ctx, int i, unsigned long token, fd_gargs const * g ) {
  fd_slot & sl = ctx->slot[i];
  hipStream_t st = ctx->stream;
  if( sl.mode==2 ) {   /* in place: one upload of the caller's region range, no host copy */
    HIPCHK( hipMemcpyAsync( sl.d_payload, sl.ref_base + sl.ref_lo, sl.payload_used + FD_ARENA_SLACK, hipMemcpyHostToDevice, st ), -2 );
  } else if( sl.mode==3 ) {   /* gathered: the rest of the records, then this stream waits for every gather */
    if( g && gather_issue( ctx, g ) ) return -2;
    HIPCHK( hipEventRecord( ctx->gev, ctx->gstream ), -2 );
    HIPCHK( hipStreamWaitEvent( st, ctx->gev, 0 ), -2 );
  } else {
    HIPCHK( hipMemcpyAsync( sl.d_payload, sl.h_payload, sl.payload_used + FD_ARENA_SLACK, hipMemcpyHostToDevice, st ), -2 );
  }
  if( sl.mode ) {
    /* raw batches: the parse kernel reads the descriptors from pinned host memory and stamps the start,
       fd_finish_kernel writes every result into pinned host memory -- four kernels fewer on the batch's
       chain than with the upload, stamp, expand and the result copies */
    int rc = launch_raw( ctx, sl.d_payload, (fdgpu_txn_raw_t const *)sl.hd_desc, sl.txn_cnt, sl.sig_cnt, sl.d_txn_out,
                         sl.d_img, FDGPU_TXN_IMG_STRIDE, sl.d_fp, st, ctx->dedup ? (u64 *)sl.d_dtag : (u64 *)NULL,
                         sl.mode==3 ? sl.d_ovr : (unsigned char const *)NULL, 1, ctx->d_stamp + 2*i );
    if( rc ) return rc;
    unsigned tg = (unsigned)( ( sl.txn_cnt + FD_WG - 1 ) / FD_WG );
    unsigned ig = (unsigned)( ( sl.txn_cnt + FD_WG/64 - 1 ) / ( FD_WG/64 ) );
    hipLaunchKernelGGL( fd_finish_kernel, dim3(tg + ig), dim3(FD_WG), 0, st, ctx->d_rdesc, (fdgpu_txn_raw_t const *)sl.hd_desc,
                        (u32)sl.txn_cnt, (u32)sl.sig_cnt, ctx->d_code, ctx->d_pflag, sl.d_fp,
                        ctx->dedup ? (u64 const *)sl.d_dtag : (u64 const *)NULL, sl.d_img, (u32)FDGPU_TXN_IMG_STRIDE,
                        sl.hd_txn_out, sl.hd_fp, ctx->dedup ? (u64 *)sl.hd_dtag : (u64 *)NULL,
                        sl.mode==3 && !sl.per_rec ? sl.ref_dev + sl.ref_lo : (unsigned char *)NULL, ctx->rec_fp_off,
                        sl.mode==3 ? (unsigned char *)NULL : sl.hd_img, tg,
                        sl.mode==3 && ctx->gather_nowb == 2 ? (unsigned char const *)sl.d_payload : (unsigned char const *)NULL,
                        sl.mode==3 && sl.per_rec ? (fd_gather const *)sl.g_dev : (fd_gather const *)NULL );
    HIPCHK( hipGetLastError(), -2 );
  } else {
    HIPCHK( hipMemcpyAsync( sl.d_desc, sl.h_desc, sl.txn_cnt * sizeof(fdgpu_txn_desc_t), hipMemcpyHostToDevice, st ), -2 );
    hipLaunchKernelGGL( fd_stamp_kernel, dim3(1), dim3(1), 0, st, ctx->d_stamp + 2*i );
    int rc = launch_batch( ctx, sl.d_payload, sl.d_desc, sl.txn_cnt, sl.sig_cnt, sl.d_txn_out, NULL, st );
    if( rc ) return rc;
    HIPCHK( hipMemcpyAsync( sl.h_txn_out, sl.d_txn_out, sl.txn_cnt, hipMemcpyDeviceToHost, st ), -2 );
  }
  hipLaunchKernelGGL( fd_done_kernel, dim3(1), dim3(1), 0, st, ctx->d_flag + i, token, ctx->d_stamp + 2*i + 1 );
  HIPCHK( hipGetLastError(), -2 );
  HIPCHK( hipEventRecord( sl.done, st ), -2 );
  return 0;
}

static int slot_launch_( fdgpu_ed25519_ctx_t * ctx, int i ) {
  fd_slot & sl = ctx->slot[i];
  fd_lcmd c;
  c.has_g = 0;
  if( sl.mode==3 ) {            /* the batch's last gather (this one, or the last early copy): phase timing */
    long n = gather_prep( ctx, sl, &c.g );
    if( n < 0 ) return (int)n;
    c.has_g = n > 0;
    sl.gt_idx = ctx->last_gt; sl.gt_target = ctx->g_launched;
  } else {
    sl.gt_idx = -1;
    if( sl.mode != 2 ) memset( sl.h_payload + sl.payload_used, 0, FD_ARENA_SLACK );
  }
  ctx->h_stamp[ 2*i ] = 0UL; ctx->h_stamp[ 2*i + 1 ] = 0UL;
  unsigned long token = sl.token + 1UL;
  if( ctx->launcher ) {
    c.ctx = ctx; c.kind = 1; c.slot = i; c.token = token;
    launcher_push( ctx->launcher, c );
  } else {
    int rc = slot_issue( ctx, i, token, c.has_g ? &c.g : NULL );
    if( rc ) return rc;
  }
  sl.token = token;
  sl.state = 1; sl.cursor = 0; sl.path = pick_path( ctx, sl.sig_cnt );
  sl.launch_ns = sl.last_query = fd_now_ns();
  ctx->n_batches++; ctx->n_txns += sl.txn_cnt;
  ctx->inflight.push_back( i );
  return 0;
}
static int slot_launch( fdgpu_ed25519_ctx_t * ctx, int i ) {
  unsigned long t0 = fd_now_ns();
  int rc = slot_launch_( ctx, i );
  ctx->launch_ns += fd_now_ns() - t0;
  return rc;
}

/* make ctx->cur a free slot; -2 if every slot is in flight, -3 if its
   buffers cannot be allocated */
static int next_free( fdgpu_ed25519_ctx_t * ctx ) {
  for( int k=0; k<FD_NSLOT; k++ ) {
    int i = (ctx->cur + k) % FD_NSLOT;
    if( ctx->slot[i].state==0 ) {
      if( slot_bufs( ctx, i ) ) return -3;
      ctx->cur = i; return 0;
    }
  }
  return -2;
}

extern "C" int
fdgpu_ed25519_flush( fdgpu_ed25519_ctx_t * ctx ) {
  fd_slot & sl = ctx->slot[ ctx->cur ];
  if( sl.state!=0 || sl.txn_cnt==0 ) return 0;
  HIPCHK( hipSetDevice( ctx->device ), -2 );
  int rc = slot_launch( ctx, ctx->cur );
  if( rc ) return rc;
  next_free( ctx );
  return 0;
}

/* the filling slot, flushed first if it cannot take one more transaction
   of payload_sz bytes / sig_cnt signatures in `mode` */
static fd_slot * slot_for( fdgpu_ed25519_ctx_t * ctx, unsigned long payload_sz, unsigned long sig_cnt, int mode, int * rc ) {
  *rc = 0;
  if( ctx->fault ) { fd_err = "ctx faulted (see the poll error); delete and recreate it"; *rc = -3; return NULL; }
  if( !ctx->slot[0].h_payload ) { fd_err = "ctx has no staging buffers (max_payload_bytes==0)"; *rc = -3; return NULL; }
  if( ( *rc = next_free( ctx ) ) ) return NULL;
  /* a record that cannot fit an empty slot's arena is refused outright (it
     would overrun the staging and device arenas) */
  if( payload_sz + 8UL > ctx->max_payload ) { fd_err = "record larger than the ctx payload arena"; *rc = FDGPU_ERR_TOO_LONG; return NULL; }
  fd_slot * sl = &ctx->slot[ ctx->cur ];
  if( sl->txn_cnt && ( sl->mode != mode || sl->txn_cnt + 1 > ctx->max_txn || sl->sig_cnt + sig_cnt > ctx->max_sig
                       || sl->payload_used + payload_sz + 8 > ctx->max_payload ) ) {
    if( ( *rc = fdgpu_ed25519_flush( ctx ) ) ) return NULL;
    if( ( *rc = next_free( ctx ) ) ) return NULL;
    sl = &ctx->slot[ ctx->cur ];
  }
  if( sl->txn_cnt==0 ) sl->mode = mode;
  return sl;
}

extern "C" int
fdgpu_ed25519_submit( fdgpu_ed25519_ctx_t * ctx, unsigned char const * payload, unsigned short payload_sz,
                      unsigned char signature_off, unsigned short acct_addr_off, unsigned short message_off,
                      unsigned char sig_cnt, unsigned long tag ) {
  int rc; fd_slot * sl = slot_for( ctx, payload_sz, sig_cnt, 0, &rc );
  if( !sl ) return rc;
  size_t off = sl->payload_used;
  memcpy( sl->h_payload + off, payload, payload_sz );
  fdgpu_txn_desc_t & d = sl->h_desc[ sl->txn_cnt ];
  d.payload_off = (unsigned)off; d.sig_base = (unsigned)sl->sig_cnt; d.payload_sz = payload_sz;
  d.message_off = message_off; d.acct_addr_off = acct_addr_off; d.signature_off = signature_off; d.sig_cnt = sig_cnt;
  sl->h_tags[ sl->txn_cnt ] = tag;
  sl->txn_cnt++; sl->sig_cnt += sig_cnt; sl->payload_used = (off + payload_sz + 7) & ~(size_t)7;
  int malformed = sig_cnt==0 || sig_cnt>16 || (unsigned)signature_off + 64u*sig_cnt > payload_sz
               || (unsigned)acct_addr_off + 32u*sig_cnt > payload_sz || message_off > payload_sz;
  return malformed ? -1 : 0;
}

static int slot_raw_bufs( fdgpu_ed25519_ctx_t * ctx, fd_slot * sl ) {
  if( sl->h_img ) return 0;
  HIPCHK( hipSetDevice( ctx->device ), -3 );
  HIPCHK( ctx_pin_alloc( ctx, &sl->h_img, ctx->max_txn * FDGPU_TXN_IMG_STRIDE, &sl->hd_img ), -3 );
  HIPCHK( ctx_pin_alloc( ctx, &sl->h_fp, ctx->max_txn * sizeof(unsigned short), &sl->hd_fp ), -3 );
  HIPCHK( ctx_dev_alloc( ctx, &sl->d_img, ctx->max_txn * FDGPU_TXN_IMG_STRIDE ), -3 );
  HIPCHK( ctx_dev_alloc( ctx, &sl->d_fp, ctx->max_txn * sizeof(unsigned short) ), -3 );
  HIPCHK( ctx_pin_alloc( ctx, &sl->h_dtag, ctx->max_txn * sizeof(unsigned long), &sl->hd_dtag ), -3 );
  HIPCHK( ctx_dev_alloc( ctx, &sl->d_dtag, ctx->max_txn * sizeof(unsigned long) ), -3 );
  HIPCHK( ctx_pin_alloc( ctx, &sl->h_gat, ctx->max_txn * sizeof(fd_gather), &sl->g_dev ), -3 );
  HIPCHK( ctx_dev_alloc( ctx, &sl->d_ovr, ctx->max_txn ), -3 );
  return 0;
}

/* every allocation the async pipeline would make on first use, now (a tile's privileged init: after
   it, batches make no allocation syscalls -- tools/sandbox/vtile_sandbox.c) */
extern "C" int
fdgpu_ed25519_prepare( fdgpu_ed25519_ctx_t * ctx, int raw ) {
  if( !ctx ) return -1;
  for( int i=0; i<FD_NSLOT; i++ ) {
    if( slot_bufs( ctx, i ) ) return -3;
    if( raw && slot_raw_bufs( ctx, &ctx->slot[i] ) ) return -3;
  }
  if( raw && gather_init( ctx ) ) return -3;
  return 0;
}

extern "C" void
fdgpu_ed25519_ctx_delete( fdgpu_ed25519_ctx_t * ctx ) {
  if( !ctx ) return;
  (void)hipSetDevice( ctx->device );
  if( ctx->launcher ) launcher_drain( ctx->launcher );   /* its queued calls are made before the streams drain */
  /* every stream of the context drains before anything is freed: gathers of a slot that was still filling
     (early copies, never launched) read its pinned descriptors and write its arena on the gather stream */
  if( ctx->gstream ) (void)hipStreamSynchronize( ctx->gstream );
  if( ctx->cstream ) (void)hipStreamSynchronize( ctx->cstream );
  if( ctx->stream ) (void)hipStreamSynchronize( ctx->stream );
  for( void * p : ctx->dev_mem ) (void)hipFree( p );
  for( void * p : ctx->pin_mem ) (void)hipHostFree( p );
  for( int i=0; i<5; i++ ) if( ctx->ev[i] ) (void)hipEventDestroy( ctx->ev[i] );
  for( int r=0; r<FD_NRING; r++ ) for( int i=0; i<5; i++ ) if( ctx->ring[r][i] ) (void)hipEventDestroy( ctx->ring[r][i] );
  for( int i=0; i<FD_NSLOT; i++ ) if( ctx->slot[i].done ) (void)hipEventDestroy( ctx->slot[i].done );
  if( ctx->cstream ) { (void)hipStreamSynchronize( ctx->cstream ); (void)hipStreamDestroy( ctx->cstream ); }
  if( ctx->gstream ) { (void)hipStreamSynchronize( ctx->gstream ); (void)hipStreamDestroy( ctx->gstream ); }
  if( ctx->gev ) (void)hipEventDestroy( ctx->gev );
  for( unsigned long i=0; i<FD_PIPE_MAX; i++ ) if( ctx->pipe_ev[i] ) (void)hipEventDestroy( ctx->pipe_ev[i] );
  if( ctx->stream ) (void)hipStreamDestroy( ctx->stream );
  delete ctx;
}

extern "C" fdgpu_ed25519_ctx_t *
fdgpu_ed25519_ctx_new( int device, unsigned long max_txn, unsigned long max_sig,
                       unsigned long max_payload_bytes, int semantics ) {
  if( max_txn==0 || max_txn >= (1UL<<24) || max_sig==0 || max_sig >= (1UL<<31) ) { fd_err = "bad sizes"; return NULL; }
  if( semantics!=FDGPU_SEMANTICS_AVX512 && semantics!=FDGPU_SEMANTICS_REF ) { fd_err = "bad semantics"; return NULL; }
  HIPCHK( hipSetDevice( device ), NULL );
  fdgpu_ed25519_ctx_t * ctx = new fdgpu_ed25519_ctx_t();
  if( ctx_init( ctx, device, max_txn, max_sig, max_payload_bytes, semantics ) ) {
    std::string err = fd_err;
    fdgpu_ed25519_ctx_delete( ctx );
    fd_err = err;
    return NULL;
  }
  return ctx;
}

/* one more raw record in the filling slot, its payload at arena offset off; the caller accounts the arena */
static inline fdgpu_txn_raw_t &
raw_append( fd_slot * sl, size_t off, unsigned short payload_sz, unsigned lanes, unsigned long tag ) {
  fdgpu_txn_raw_t & r = ((fdgpu_txn_raw_t *)sl->h_desc)[ sl->txn_cnt ];
  r.payload_off = (unsigned)off; r.sig_base = (unsigned)sl->sig_cnt; r.payload_sz = payload_sz; r.sig_lanes = (unsigned char)lanes;
  sl->h_tags[ sl->txn_cnt ] = tag;
  sl->txn_cnt++; sl->sig_cnt += lanes;
  return r;
}

extern "C" int
fdgpu_ed25519_submit_raw( fdgpu_ed25519_ctx_t * ctx, unsigned char const * payload, unsigned short payload_sz,
                          unsigned long tag ) {
  unsigned lanes = raw_lanes( payload, payload_sz );
  int rc; fd_slot * sl = slot_for( ctx, payload_sz, lanes, 1, &rc );
  if( !sl ) return rc;
  if( slot_raw_bufs( ctx, sl ) ) return -3;
  size_t off = sl->payload_used;
  memcpy( sl->h_payload + off, payload, payload_sz );
  raw_append( sl, off, payload_sz, lanes, tag );
  sl->payload_used = (off + payload_sz + 7) & ~(size_t)7;
  return 0;
}

/* In-place raw submission: the payload already sits in a pinned host
   region the caller owns (the tile's out dcache, allocated with
   fdgpu_host_alloc); a batch uploads the contiguous range of its
   payloads straight from there.  Payloads of one batch must be at
   increasing addresses in one region (a ring wrap simply starts a new
   batch), with 512 readable bytes after each. */
extern "C" int
fdgpu_ed25519_submit_raw_ref( fdgpu_ed25519_ctx_t * ctx, unsigned char const * base, unsigned char const * payload,
                              unsigned short payload_sz, unsigned long tag ) {
  unsigned lanes = raw_lanes( payload, payload_sz );
  size_t off = (size_t)( payload - base );
  int rc; fd_slot * sl = slot_for( ctx, payload_sz, lanes, 2, &rc );
  if( !sl ) return rc;
  if( sl->txn_cnt && ( sl->ref_base != base || off < sl->ref_hi || off + payload_sz - sl->ref_lo + 8UL > ctx->max_payload ) ) {
    if( ( rc = fdgpu_ed25519_flush( ctx ) ) ) return rc;
    if( !( sl = slot_for( ctx, payload_sz, lanes, 2, &rc ) ) ) return rc;
  }
  if( slot_raw_bufs( ctx, sl ) ) return -3;
  if( !sl->txn_cnt ) { sl->ref_base = base; sl->ref_lo = off; }
  raw_append( sl, off - sl->ref_lo, payload_sz, lanes, tag );
  sl->ref_hi = off + payload_sz; sl->payload_used = sl->ref_hi - sl->ref_lo;
  return 0;
}

/* The writers of the region table (g_regions, above region_dev) */
static void region_add_locked( void * h, void * d, unsigned long sz ) {
  int n = g_region_cnt.load( std::memory_order_relaxed ), i = 0;
  while( i < n && g_regions[i].sz.load( std::memory_order_relaxed ) ) i++;     /* reuse a removed entry */
  if( i == FD_REGION_MAX ) return;
  g_regions[i].h = (unsigned char const *)h; g_regions[i].d = (unsigned char *)d; g_regions[i].refs = 1; g_regions[i].shared = 0;
  g_regions[i].sz.store( sz, std::memory_order_release );
  if( i == n ) g_region_cnt.store( n + 1, std::memory_order_release );
}
static void region_add( void * h, void * d, unsigned long sz ) {
  std::lock_guard<std::mutex> lk( g_reg_mu );
  region_add_locked( h, d, sz );
}
/* the live entry starting at h (-1: none); under g_reg_mu */
static int region_find_locked( void const * h ) {
  int n = g_region_cnt.load( std::memory_order_relaxed );
  for( int i=0; i<n; i++ )
    if( g_regions[i].h == (unsigned char const *)h && g_regions[i].sz.load( std::memory_order_relaxed ) ) return i;
  return -1;
}
static void region_del( void * h ) {
  std::lock_guard<std::mutex> lk( g_reg_mu );
  int i = region_find_locked( h );
  if( i >= 0 ) g_regions[i].sz.store( 0UL, std::memory_order_release );
}
/* the registered region holding p: its host base, size and device base (0), or -1 */
extern "C" int
fdgpu_host_region( void const * p, void ** base, unsigned long * sz, void ** dev_base ) {
  unsigned char const * q = (unsigned char const *)p;
  int n = g_region_cnt.load( std::memory_order_acquire );
  for( int i=0; i<n; i++ ) {
    unsigned long rs = g_regions[i].sz.load( std::memory_order_acquire );
    unsigned char const * h = g_regions[i].h;
    if( rs && q >= h && q < h + rs ) { *base = (void *)h; *sz = rs; *dev_base = g_regions[i].d; return 0; }
  }
  return -1;
}

extern "C" void *
fdgpu_host_alloc( unsigned long sz ) {
  void * p = NULL;
  if( hipHostMalloc( &p, sz, hipHostMallocDefault ) != hipSuccess ) { fd_err = "hipHostMalloc failed"; return NULL; }
  void * d = NULL;
  if( hipHostGetDevicePointer( &d, p, 0 ) == hipSuccess ) region_add( p, d, sz );
  return p;
}

extern "C" void fdgpu_host_free( void * p ) { if( p ) { region_del( p ); hipHostFree( p ); } }

static int host_register_locked( void * p, unsigned long sz, int shared ) {
  HIPCHK( hipHostRegister( p, sz, hipHostRegisterMapped ), -2 );
  void * d = NULL;
  hipError_t e = hipHostGetDevicePointer( &d, p, 0 );
  if( e != hipSuccess ) { set_err( "hipHostGetDevicePointer", e ); (void)hipHostUnregister( p ); return -2; }
  region_add_locked( p, d, sz );
  int i = region_find_locked( p );
  if( i >= 0 ) g_regions[i].shared = shared;
  return 0;
}

extern "C" int
fdgpu_host_register( void * p, unsigned long sz ) {
  if( !p || !sz ) { fd_err = "fdgpu_host_register: empty range"; return -1; }
  std::lock_guard<std::mutex> lk( g_reg_mu );
  if( region_find_locked( p ) >= 0 ) { fd_err = "fdgpu_host_register: a range starting there is registered"; return -2; }
  return host_register_locked( p, sz, 0 );
}

/* Holders that share one range (the verify tiles' handles on one mcache ring, fdgpu_vtile_set_in_links):
   the first registers it, later ones with exactly the same (p, sz) take a reference, and the range is
   unmapped at the last fdgpu_host_unregister.  A range an owner registered with fdgpu_host_register is
   never shared: 1 (nothing taken, the owner keeps it mapped). */
extern "C" int
fdgpu_host_register_shared( void * p, unsigned long sz ) {
  if( !p || !sz ) { fd_err = "fdgpu_host_register_shared: empty range"; return -1; }
  std::lock_guard<std::mutex> lk( g_reg_mu );
  int i = region_find_locked( p );
  if( i >= 0 ) {
    if( g_regions[i].sz.load( std::memory_order_relaxed ) != sz ) {
      fd_err = "fdgpu_host_register_shared: another range starting there is registered"; return -2;
    }
    if( !g_regions[i].shared ) return 1;
    g_regions[i].refs++;
    return 0;
  }
  return host_register_locked( p, sz, 1 );
}

extern "C" void
fdgpu_host_unregister( void * p ) {
  if( !p ) return;
  std::lock_guard<std::mutex> lk( g_reg_mu );
  int i = region_find_locked( p );
  if( i < 0 ) return;
  if( g_regions[i].shared && --g_regions[i].refs > 0 ) return;
  g_regions[i].sz.store( 0UL, std::memory_order_release );
  (void)hipHostUnregister( p );
}

extern "C" int
fdgpu_device_numa_node( int device ) {
  char bus[ 64 ];
  if( hipDeviceGetPCIBusId( bus, (int)sizeof(bus), device ) != hipSuccess ) return -1;
  for( char * c = bus; *c; c++ ) if( *c >= 'A' && *c <= 'F' ) *c = (char)( *c - 'A' + 'a' );
  char path[ 128 ];
  snprintf( path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bus );
  FILE * f = fopen( path, "r" );
  if( !f ) return -1;
  int node = -1;
  if( fscanf( f, "%d", &node ) != 1 ) node = -1;
  fclose( f );
  return node;
}

/* Gathered raw submission: the record (copy_sz bytes at src, the payload
   at src + payload_off) stays where the caller's producer wrote it, in a
   registered host region; the batch's gather kernel copies it into the
   device arena and into dst, the record's place in the caller's pinned
   out region dst_base.  Records of one batch lie at increasing dst
   addresses (a lower one starts a new batch), chunk aligned. */
static int submit_gather( fdgpu_ed25519_ctx_t * ctx, unsigned char const * src, unsigned char const * dsrc,
                          unsigned char * dst_base, unsigned char * dst, unsigned long csz, unsigned short payload_off,
                          unsigned short payload_sz, unsigned long tag, unsigned char const * dseq, unsigned long seq,
                          unsigned flags ) {
  unsigned lanes = raw_lanes( src + payload_off, payload_sz );
  /* per-record (dst_base NULL): the record goes back to dst_dev, a place of its own; its arena offset is
     the next free one of the batch.  Else its arena offset mirrors its offset in the batch's out region. */
  int per_rec = !dst_base;
  size_t off = per_rec ? 0UL : (size_t)( dst - dst_base );
  int rc; fd_slot * sl = slot_for( ctx, csz, lanes, 3, &rc );
  if( !sl ) return rc;
  if( sl->txn_cnt && ( sl->per_rec != per_rec ||
                       ( !per_rec && ( sl->ref_base != dst_base || off < sl->ref_hi ||
                                       off + csz - sl->ref_lo + 8UL > ctx->max_payload ) ) ) ) {
    if( ( rc = fdgpu_ed25519_flush( ctx ) ) ) return rc;
    if( !( sl = slot_for( ctx, csz, lanes, 3, &rc ) ) ) return rc;
  }
  if( slot_raw_bufs( ctx, sl ) ) return -3;
  if( !sl->txn_cnt ) {
    sl->per_rec = per_rec;
    if( per_rec ) { sl->ref_base = NULL; sl->ref_dev = NULL; sl->ref_lo = 0UL; sl->ref_hi = 0UL; }
    else {
      unsigned char * d = region_dev( dst_base, 1UL );
      if( !d ) { fd_err = "fdgpu_ed25519_submit_raw_gather: dst_base not from fdgpu_host_alloc"; return -3; }
      sl->ref_base = dst_base; sl->ref_dev = d; sl->ref_lo = off;
    }
  }
  if( per_rec ) off = sl->ref_hi;                /* (arena offsets stay 16-B aligned: csz is) */
  fd_gather & g = sl->h_gat[ sl->txn_cnt ];
  fdgpu_txn_raw_t & r = raw_append( sl, off - sl->ref_lo + payload_off, payload_sz, lanes, tag );
  r._pad[0] = (unsigned char)payload_off;      /* fd_img_scatter_kernel finds the record header from it */
  r._pad[1] = (unsigned char)( ( flags >> 8 ) & 15u );   /* its HA dedup seed (FDGPU_GATHER_SEED) */
  g.src = (unsigned long)dsrc; g.dst = (unsigned)( off - sl->ref_lo );
  /* a per-record batch writes its records back at the gather unless the write-back is off or deferred to the
     finish kernel (fdgpu_debug_opts_t.gather_no_writeback, whose A/B applies to both forms) */
  unsigned nowb = ( flags & FDGPU_GATHER_NO_WRITEBACK ) || ( per_rec && ctx->gather_nowb );
  g.sz = (unsigned)csz | ( nowb ? 0x80000000u : 0u );
  g.seq_addr = (unsigned long)dseq; g.seq = seq;
  g.wb = per_rec ? (unsigned long)dst : 0UL;
  sl->ref_hi = off + csz; sl->payload_used = sl->ref_hi - sl->ref_lo;
  return 0;
}

/* The record check of every gathered submit, on the tile's thread once per frag: the payload inside the
   copied bytes; src, its device view and the record's place (place: its offset in the out region, or in the
   per-record form its device address, which must be given) 16-byte aligned; the seq word 8-byte aligned; the
   footprint field (fdgpu_ed25519_set_record_fp_off) inside the header ahead of the payload; no flag outside
   flags_ok.  src_dev is NULL where the caller has not looked it up yet.  0, or -1 with fd_err set. */
static inline int
gather_check( fdgpu_ed25519_ctx_t const * ctx, void const * src, void const * src_dev, uintptr_t place, int per_rec,
              void const * seq, unsigned copy_sz, unsigned payload_off, unsigned payload_sz, unsigned flags,
              unsigned flags_ok ) {
  if( payload_off + payload_sz > copy_sz || ( (uintptr_t)src & 15 ) || ( (uintptr_t)src_dev & 15 ) ||
      ( per_rec && !place ) || ( place & 15 ) ||
      ( ctx->rec_fp_off >= 0 && ( payload_off > 255u || (unsigned)ctx->rec_fp_off + 2u > payload_off ) ) ||
      ( (uintptr_t)seq & 7 ) || ( flags & ~flags_ok ) ) {
    fd_err = per_rec ? "fdgpu_ed25519_submit_raw_gather_to: bad record" : "fdgpu_ed25519_submit_raw_gather: bad record";
    return -1;
  }
  return 0;
}
#define FD_GATHER_CSZ( copy_sz ) ( ( (unsigned long)(copy_sz) + 15UL ) & ~15UL )   /* the bytes copied: whole 16-B chunks */

extern "C" int
fdgpu_ed25519_submit_raw_gather_chk( fdgpu_ed25519_ctx_t * ctx, unsigned char const * src, unsigned char * dst_base,
                                     unsigned char * dst, unsigned short copy_sz, unsigned short payload_off,
                                     unsigned short payload_sz, unsigned long tag, unsigned long const * seq_addr,
                                     unsigned long seq ) {
  if( gather_check( ctx, src, NULL, (uintptr_t)( dst - dst_base ), 0, seq_addr, copy_sz, payload_off, payload_sz, 0u, 0u ) )
    return -1;
  unsigned long csz = FD_GATHER_CSZ( copy_sz );
  unsigned char * dsrc = region_dev( src, csz );
  if( !dsrc ) { fd_err = "fdgpu_ed25519_submit_raw_gather: src not in a registered region"; return -3; }
  unsigned char * dseq = NULL;
  if( seq_addr && !( dseq = region_dev( seq_addr, sizeof(unsigned long) ) ) ) {
    fd_err = "fdgpu_ed25519_submit_raw_gather: seq_addr not in a registered region"; return -3;
  }
  return submit_gather( ctx, src, dsrc, dst_base, dst, csz, payload_off, payload_sz, tag, dseq, seq, 0u );
}

/* the same with the device addresses of src and seq_addr already known to the caller (a tile that
   translated its in link's regions once, fdgpu_host_dev_ptr): no region lookup per frag.  The only flag
   is FDGPU_GATHER_NO_WRITEBACK: a dedup seed goes with the per-record form alone. */
extern "C" int
fdgpu_ed25519_submit_raw_gather_dev_f( fdgpu_ed25519_ctx_t * ctx, unsigned char const * src, unsigned char const * src_dev,
                                       unsigned char * dst_base, unsigned char * dst, unsigned short copy_sz,
                                       unsigned short payload_off, unsigned short payload_sz, unsigned long tag,
                                       unsigned long const * seq_dev, unsigned long seq, unsigned flags ) {
  if( gather_check( ctx, src, src_dev, (uintptr_t)( dst - dst_base ), 0, seq_dev, copy_sz, payload_off, payload_sz, flags,
                    FDGPU_GATHER_NO_WRITEBACK ) ) return -1;
  return submit_gather( ctx, src, src_dev, dst_base, dst, FD_GATHER_CSZ( copy_sz ), payload_off, payload_sz, tag,
                        (unsigned char const *)seq_dev, seq, flags );
}

extern "C" int
fdgpu_ed25519_submit_raw_gather_dev( fdgpu_ed25519_ctx_t * ctx, unsigned char const * src, unsigned char const * src_dev,
                                     unsigned char * dst_base, unsigned char * dst, unsigned short copy_sz,
                                     unsigned short payload_off, unsigned short payload_sz, unsigned long tag,
                                     unsigned long const * seq_dev, unsigned long seq ) {
  return fdgpu_ed25519_submit_raw_gather_dev_f( ctx, src, src_dev, dst_base, dst, copy_sz, payload_off, payload_sz, tag,
                                                seq_dev, seq, 0u );
}

/* the per-record form (dst_base NULL selects it in submit_gather; dst carries the device address), which
   also admits a dedup seed (FDGPU_GATHER_SEED) */
extern "C" int
fdgpu_ed25519_submit_raw_gather_to( fdgpu_ed25519_ctx_t * ctx, unsigned char const * src, unsigned char const * src_dev,
                                    unsigned char * dst_dev, unsigned short copy_sz, unsigned short payload_off,
                                    unsigned short payload_sz, unsigned long tag, unsigned long const * seq_dev,
                                    unsigned long seq, unsigned flags ) {
  if( gather_check( ctx, src, src_dev, (uintptr_t)dst_dev, 1, seq_dev, copy_sz, payload_off, payload_sz, flags,
                    FDGPU_GATHER_NO_WRITEBACK | 0xf00u ) ) return -1;
  return submit_gather( ctx, src, src_dev, NULL, dst_dev, FD_GATHER_CSZ( copy_sz ), payload_off, payload_sz, tag,
                        (unsigned char const *)seq_dev, seq, flags );
}

extern "C" int
fdgpu_ed25519_submit_raw_gather( fdgpu_ed25519_ctx_t * ctx, unsigned char const * src, unsigned char * dst_base,
                                 unsigned char * dst, unsigned short copy_sz, unsigned short payload_off,
                                 unsigned short payload_sz, unsigned long tag ) {
  return fdgpu_ed25519_submit_raw_gather_chk( ctx, src, dst_base, dst, copy_sz, payload_off, payload_sz, tag, NULL, 0UL );
}

extern "C" long
fdgpu_ed25519_gather( fdgpu_ed25519_ctx_t * ctx ) {
  if( !ctx || ctx->fault ) return -3;
  fd_slot & sl = ctx->slot[ ctx->cur ];
  if( sl.state != 0 || sl.mode != 3 || sl.gathered == sl.txn_cnt ) return 0;
  HIPCHK( hipSetDevice( ctx->device ), -2 );
  unsigned long t0 = fd_now_ns();
  long n = gather_launch( ctx, sl );
  ctx->launch_ns += fd_now_ns() - t0;
  return n;
}

extern "C" unsigned long
fdgpu_ed25519_gathered( fdgpu_ed25519_ctx_t const * ctx ) {
  unsigned long g = ctx->h_flag[ FD_NSLOT + 1 ];
  std::atomic_thread_fence( std::memory_order_acquire );
  return g;
}

extern "C" unsigned long
fdgpu_ed25519_gather_launched( fdgpu_ed25519_ctx_t const * ctx ) { return ctx->g_launched; }

extern "C" void
fdgpu_ed25519_gather_stats( fdgpu_ed25519_ctx_t * ctx, unsigned long out[ 8 ] ) {
  gather_times( ctx, fdgpu_ed25519_gathered( ctx ) );
  out[0] = ctx->gs_n; out[1] = ctx->gs_start_sum; out[2] = ctx->gs_start_max; out[3] = ctx->gs_run_sum; out[4] = ctx->gs_run_max;
  out[5] = ctx->gs_issue_sum; out[6] = ctx->gs_issue_max; out[7] = ctx->gs_issue_slow;
}

extern "C" int
fdgpu_ed25519_reserve_gather_cus( fdgpu_ed25519_ctx_t * ctx, unsigned n ) {
  return fdgpu_ed25519_reserve_cus( ctx, n, 0u, 1u );
}

extern "C" int
fdgpu_ed25519_reserve_cus( fdgpu_ed25519_ctx_t * ctx, unsigned n, unsigned part, unsigned parts ) {
  if( !ctx || ctx->gstream || !ctx->inflight.empty() || ctx->slot[ ctx->cur ].txn_cnt ) {
    fd_err = "fdgpu_ed25519_reserve_cus: only on a fresh context"; return -1;
  }
  if( !parts || part >= parts ) { fd_err = "fdgpu_ed25519_reserve_cus: part >= parts"; return -1; }
  if( !n ) return 0;
  HIPCHK( hipSetDevice( ctx->device ), -2 );
  int ncu = 0;
  HIPCHK( hipDeviceGetAttribute( &ncu, hipDeviceAttributeMultiprocessorCount, ctx->device ), -2 );
  if( (int)n >= ncu ) { fd_err = "fdgpu_ed25519_reserve_gather_cus: n >= CUs"; return -1; }
  std::vector<uint32_t> cm( (size_t)( ncu + 31 ) / 32, 0u ), gm( cm.size(), 0u );
  /* the last n CUs (default); gather_cu_spread 1: every (ncu/n)-th CU; 2: the first n (A/B).  The
     verify kernels get the rest, or with parts > 1 the part-th of `parts` contiguous shares of the rest */
  int stride = ncu / (int)n, nrest = ncu - (int)n, i = 0;
  if( nrest < (int)parts ) { fd_err = "fdgpu_ed25519_reserve_cus: fewer CUs than parts"; return -1; }
  for( int c=0; c<ncu; c++ ) {
    int mine = ctx->gather_cu_spread == 1 ? ( c % stride == stride - 1 && c / stride < (int)n )
             : ctx->gather_cu_spread == 2 ? c < (int)n : c >= ncu - (int)n;
    if( mine ) { gm[ (size_t)c / 32 ] |= 1u << ( c % 32 ); continue; }
    if( (unsigned)( (long)i * (long)parts / (long)nrest ) == part ) cm[ (size_t)c / 32 ] |= 1u << ( c % 32 );
    i++;
  }
  hipStream_t s = NULL, g = NULL;
  HIPCHK( hipExtStreamCreateWithCUMask( &s, (uint32_t)cm.size(), cm.data() ), -2 );
  hipError_t e = hipExtStreamCreateWithCUMask( &g, (uint32_t)gm.size(), gm.data() );
  if( e != hipSuccess ) { (void)hipStreamDestroy( s ); set_err( "hipExtStreamCreateWithCUMask", e ); return -2; }
  e = hipEventCreateWithFlags( &ctx->gev, hipEventDisableTiming );
  if( e != hipSuccess ) { (void)hipStreamDestroy( s ); (void)hipStreamDestroy( g ); set_err( "hipEventCreate", e ); return -2; }
  /* HIP has no CU-masked stream with flags or a priority: both streams are blocking (they order with
     the null stream, which the tile never uses) and of default priority -- the copies' precedence over
     queued verify work comes from their reserved CUs, not from a stream priority (gather_init's
     highest-priority stream is only made when no CUs are reserved) */
  (void)hipStreamSynchronize( ctx->stream );
  (void)hipStreamDestroy( ctx->stream );
  ctx->stream = s; ctx->gstream = g; ctx->gather_cus = n;
  return 0;
}

extern "C" int
fdgpu_ed25519_gather_wait( fdgpu_ed25519_ctx_t * ctx ) {
  if( !ctx || ctx->fault ) return -3;
  if( ctx->launcher ) launcher_drain( ctx->launcher );   /* (a queued gather is not on its stream yet) */
  unsigned long t0 = fd_now_ns(), last = t0;
  while( fdgpu_ed25519_gathered( ctx ) != ctx->g_launched ) {
    unsigned long now = fd_now_ns();
    if( now - last > 2000000UL ) {        /* a failed gather never stores its count: ask the stream */
      last = now;
      hipError_t e = hipStreamQuery( ctx->gstream );
      if( e != hipSuccess && e != hipErrorNotReady ) { set_err( "fdgpu_ed25519_gather_wait", e ); ctx->fault = 1; return -3; }
      if( e == hipSuccess && fdgpu_ed25519_gathered( ctx ) != ctx->g_launched ) { fd_err = "gather count lost"; return -2; }
    }
    __builtin_ia32_pause();
  }
  return 0;
}

extern "C" void *
fdgpu_host_dev_ptr( void const * p, unsigned long sz ) { return region_dev( p, sz ); }

/* Phases of a completed batch (fdgpu_ed25519_phase_stats), from the GPU clock stamps converted to host
   time: launch -> its verify kernels start (its gathers, the stream's previous batch), start -> end,
   end -> the host sees it, and launch -> its last gather ends (gathered batches). */
static void phase_max( unsigned long * m, double v ) { if( v > (double)*m ) *m = (unsigned long)v; }
static void phase_account( fdgpu_ed25519_ctx_t * ctx, int i, unsigned long now ) {
  fd_slot const & sl = ctx->slot[i];
  unsigned long s0 = ctx->h_stamp[ 2*i ], s1 = ctx->h_stamp[ 2*i + 1 ];
  if( !ctx->gclk_ok || !s0 || s1 < s0 ) return;
  double l = (double)sl.launch_ns, t0 = (double)s0 * 10.0 - ctx->gclk_off_ns, t1 = (double)s1 * 10.0 - ctx->gclk_off_ns;
  double a = t0 > l ? t0 - l : 0., c = t1 - t0, r = (double)now > t1 ? (double)now - t1 : 0.;
  unsigned long * ph = ctx->ph;
  ph[0]++; ph[1] += (unsigned long)a; phase_max( &ph[2], a );
  ph[3] += (unsigned long)c; phase_max( &ph[4], c );
  ph[5] += (unsigned long)r; phase_max( &ph[6], r );
  if( sl.mode == 3 && sl.gt_idx >= 0 && ctx->gt[ sl.gt_idx ].target == sl.gt_target ) {
    unsigned long ge = ctx->h_gtime[ 2*sl.gt_idx + 1 ];
    if( ge ) {
      double g = (double)ge * 10.0 - ctx->gclk_off_ns - l;
      ph[7] += g > 0. ? (unsigned long)g : 0UL; ph[8]++;
    }
  }
}

extern "C" void
fdgpu_ed25519_phase_stats( fdgpu_ed25519_ctx_t const * ctx, unsigned long out[ 9 ] ) {
  memcpy( out, ctx->ph, sizeof(ctx->ph) );
}

/* Drain completed slots in submission order, at most max results. */
static unsigned long
poll_any( fdgpu_ed25519_ctx_t * ctx, unsigned long * out_tags, signed char * out_codes, unsigned char * out_img,
          unsigned short * out_fp, unsigned long * out_dtag, unsigned long max, int blocking ) {
  if( ctx->fault ) {                     /* faulted: nothing more completes (never block on it) */
    if( ctx->lerr[0] ) fd_err = ctx->lerr;
    return 0;
  }
  unsigned long n = 0;
  while( n < max && !ctx->inflight.empty() ) {
    int i = ctx->inflight.front();
    fd_slot & sl = ctx->slot[i];
    if( sl.cursor==0 ) {
      /* ready when fd_done_kernel has stored the slot's token; a batch that failed never
         stores it, so the stream's event is asked (a HIP call, with runtime locks) only
         after 2 ms without the token and then once per ms */
      int ready = 0;
      for(;;) {
        if( ctx->h_flag[i] == sl.token ) { ready = 1; break; }
        /* the context's launch thread faults it when one of its calls fails, and the batch's done kernel and
           event are then never issued: the token never comes and the event (unrecorded, or still holding the
           slot's previous batch) reads complete -- so a blocking wait must see that fault itself */
        if( __atomic_load_n( &ctx->fault, __ATOMIC_ACQUIRE ) ) break;
        unsigned long now = fd_now_ns();
        if( now - sl.launch_ns > 2000000UL && now - sl.last_query > 1000000UL ) {
          sl.last_query = now;
          (void)hipSetDevice( ctx->device );   /* (only here: the poll itself reads host memory) */
          hipError_t e = hipEventQuery( sl.done );
          if( e != hipSuccess && e != hipErrorNotReady ) { set_err( "fdgpu_ed25519_poll: batch failed", e ); ctx->fault = 1; break; }
          if( e == hipSuccess && ctx->h_flag[i] == sl.token ) { ready = 1; break; }
        }
        if( !blocking ) break;
        __builtin_ia32_pause();
      }
      if( __atomic_load_n( &ctx->fault, __ATOMIC_ACQUIRE ) ) { if( ctx->lerr[0] ) fd_err = ctx->lerr; break; }
      if( !ready ) break;
      std::atomic_thread_fence( std::memory_order_acquire );
      unsigned long now = fd_now_ns();
      ctx->lat_hist[ fdgpu_lat_bucket( now - sl.launch_ns ) ]++;
      phase_account( ctx, i, now );
    }
    unsigned long k = sl.txn_cnt - sl.cursor;
    if( k > max - n ) k = max - n;
    unsigned long pf = (unsigned long)ctx->poll_pf;
    /* the slot's arrays in locals: the out arrays could alias them as far as the compiler knows, which
       would reload every field of the slot on every iteration */
    unsigned long const * __restrict__ h_tags = sl.h_tags;
    signed char const *   __restrict__ h_out  = (signed char const *)sl.h_txn_out;
    unsigned short const * __restrict__ h_fp  = sl.h_fp;
    unsigned long const * __restrict__ h_dtag = sl.h_dtag;
    unsigned long const cur = sl.cursor, cnt = sl.txn_cnt;
    int const mode = sl.mode, want_dtag = sl.mode && ctx->dedup;
    for( unsigned long t=0; t<k; t++ ) {
      unsigned long u = cur + t;
      /* the result arrays were written by the GPU over PCIe: their lines are not in the CPU's caches */
      if( pf && !( u & 7UL ) && u + pf < cnt ) {
        __builtin_prefetch( h_tags + u + pf );
        if( mode ) { __builtin_prefetch( h_dtag + u + pf ); __builtin_prefetch( h_fp + u + 4*pf ); }
        __builtin_prefetch( h_out + u + 8*pf );
      }
      out_tags[n+t]  = h_tags[u];
      out_codes[n+t] = h_out[u];
      if( out_fp )  out_fp[n+t] = mode ? h_fp[u] : 0;
      if( out_dtag ) out_dtag[n+t] = want_dtag ? h_dtag[u] : 0UL;
      if( out_img && mode && mode != 3 ) {         /* mode 3: the image is in the caller's out region */
        unsigned fp = h_fp[u];
        memcpy( out_img + (n+t)*FDGPU_TXN_IMG_STRIDE, sl.h_img + u*FDGPU_TXN_IMG_STRIDE, fp );
      }
    }
    n += k; sl.cursor += k;
    if( sl.cursor==sl.txn_cnt ) {
      ctx->inflight.pop_front();
      sl.txn_cnt = 0; sl.sig_cnt = 0; sl.payload_used = 0; sl.cursor = 0; sl.state = 0; sl.gathered = 0;
    }
  }
  return n;
}

extern "C" int fdgpu_ed25519_faulted( fdgpu_ed25519_ctx_t const * ctx ) { return ctx ? ctx->fault : 1; }

extern "C" void
fdgpu_ed25519_launch_stats( fdgpu_ed25519_ctx_t const * ctx, unsigned long * launch_ns, unsigned long * launches ) {
  *launch_ns = ctx->launch_ns; *launches = ctx->n_batches;
}

extern "C" void
fdgpu_ed25519_batch_stats( fdgpu_ed25519_ctx_t const * ctx, unsigned long * batches, unsigned long * txns,
                           unsigned long hist[ FDGPU_LAT_BUCKETS ] ) {
  *batches = ctx->n_batches; *txns = ctx->n_txns;
  if( hist ) memcpy( hist, ctx->lat_hist, sizeof(ctx->lat_hist) );
}

/* host-side test hook: the context behaves exactly as after a failed batch */
extern "C" void
fdgpu_ed25519_debug_fail_launch( fdgpu_ed25519_ctx_t * ctx, int on ) {
  __atomic_store_n( &ctx->dbg_fail_issue, on ? 1 : 0, __ATOMIC_RELEASE );
}

extern "C" void
fdgpu_ed25519_debug_fault( fdgpu_ed25519_ctx_t * ctx ) {
  if( !ctx ) return;
  ctx->fault = 1;
  fd_err = "fdgpu_ed25519_poll: batch failed: injected by fdgpu_ed25519_debug_fault";
}

extern "C" unsigned long
fdgpu_ed25519_slow_count( fdgpu_ed25519_ctx_t * ctx ) {
  if( !ctx || !ctx->half ) return 0UL;
  if( hipSetDevice( ctx->device ) != hipSuccess || hipStreamSynchronize( ctx->stream ) != hipSuccess ) return ~0UL;
  u32 cnt = 0u;
  if( hipMemcpy( &cnt, slow_word( ctx, FD_SW_SLOW ), sizeof(u32), hipMemcpyDeviceToHost ) != hipSuccess ) return ~0UL;
  return (unsigned long)cnt;
}

extern "C" unsigned long
fdgpu_ed25519_key_count( fdgpu_ed25519_ctx_t * ctx ) {
  if( !ctx || !ctx->half || !ctx->key_dedup || ctx->last_path != FDGPU_PATH_THROUGHPUT ) return 0UL;
  if( hipSetDevice( ctx->device ) != hipSuccess || hipStreamSynchronize( ctx->stream ) != hipSuccess ) return ~0UL;
  u32 cnt = 0u;
  if( hipMemcpy( &cnt, slow_word( ctx, FD_SW_KEYS ), sizeof(u32), hipMemcpyDeviceToHost ) != hipSuccess ) return ~0UL;
  return (unsigned long)cnt;
}

extern "C" int
fdgpu_ed25519_hot_count( fdgpu_ed25519_ctx_t * ctx, unsigned long * hot_keys, unsigned long * hot_sigs ) {
  if( hot_keys ) *hot_keys = 0UL;
  if( hot_sigs ) *hot_sigs = 0UL;
  if( !ctx || !ctx->half || !ctx->key_split || ctx->last_path != FDGPU_PATH_THROUGHPUT ) return 0;
  if( hipSetDevice( ctx->device ) != hipSuccess || hipStreamSynchronize( ctx->stream ) != hipSuccess ) return -1;
  u32 cnt[ 5 ] = { 0u, 0u, 0u, 0u, 0u };
  if( hipMemcpy( cnt, slow_word( ctx, FD_SW_HOT ), sizeof(cnt), hipMemcpyDeviceToHost ) != hipSuccess ) return -1;
  /* the repeated keys, whichever walk they took: a fixed-base key (fdgpu_ed25519_fixed_count) is one of them */
  if( ctx->key_fixed ) { cnt[0] += cnt[FD_KC_FBK] < ctx->fb_cap ? cnt[FD_KC_FBK] : ctx->fb_cap; cnt[1] += cnt[FD_KC_FB]; }
  if( hot_keys ) *hot_keys = (unsigned long)cnt[0];
  if( hot_sigs ) *hot_sigs = (unsigned long)cnt[1];
  return 0;
}

extern "C" int
fdgpu_ed25519_fixed_count( fdgpu_ed25519_ctx_t * ctx, unsigned long * fixed_keys, unsigned long * fixed_sigs ) {
  if( fixed_keys ) *fixed_keys = 0UL;
  if( fixed_sigs ) *fixed_sigs = 0UL;
  if( !ctx || !ctx->half || !ctx->key_fixed || ctx->last_path != FDGPU_PATH_THROUGHPUT ) return 0;
  if( hipSetDevice( ctx->device ) != hipSuccess || hipStreamSynchronize( ctx->stream ) != hipSuccess ) return -1;
  u32 cnt[ 2 ] = { 0u, 0u };
  if( hipMemcpy( cnt, slow_word( ctx, FD_SW_HOT ) + FD_KC_FBK, sizeof(cnt), hipMemcpyDeviceToHost ) != hipSuccess ) return -1;
  if( cnt[0] > ctx->fb_cap ) cnt[0] = ctx->fb_cap;     /* (keys that claimed an index beyond the cap stayed hot) */
  if( fixed_keys ) *fixed_keys = (unsigned long)cnt[0];
  if( fixed_sigs ) *fixed_sigs = (unsigned long)cnt[1];
  return 0;
}

extern "C" int
fdgpu_ed25519_fcache_count( fdgpu_ed25519_ctx_t * ctx, unsigned long * hits, unsigned long * builds ) {
  if( hits ) *hits = 0UL;
  if( builds ) *builds = 0UL;
  if( !ctx || !ctx->half || !ctx->key_fixed || ctx->last_path != FDGPU_PATH_THROUGHPUT ) return 0;
  if( hipSetDevice( ctx->device ) != hipSuccess || hipStreamSynchronize( ctx->stream ) != hipSuccess ) return -1;
  u32 cnt[ 3 ] = { 0u, 0u, 0u };                         /* (hits, misses, builds) */
  if( hipMemcpy( cnt, slow_word( ctx, FD_SW_HOT ) + FD_KC_HIT, sizeof(cnt), hipMemcpyDeviceToHost ) != hipSuccess ) return -1;
  if( hits ) *hits = (unsigned long)cnt[0];
  if( builds ) *builds = (unsigned long)cnt[2];
  return 0;
}

extern "C" int
fdgpu_ed25519_ffull_count( fdgpu_ed25519_ctx_t * ctx, unsigned long * keys, unsigned long * sigs ) {
  if( keys ) *keys = 0UL;
  if( sigs ) *sigs = 0UL;
  if( !ctx || !ctx->half || !ctx->key_fixed || ctx->last_path != FDGPU_PATH_THROUGHPUT ) return 0;
  if( hipSetDevice( ctx->device ) != hipSuccess || hipStreamSynchronize( ctx->stream ) != hipSuccess ) return -1;
  u32 cnt[ 2 ] = { 0u, 0u };
  if( hipMemcpy( cnt, slow_word( ctx, FD_SW_HOT ) + FD_KC_FFK, sizeof(cnt), hipMemcpyDeviceToHost ) != hipSuccess ) return -1;
  if( keys ) *keys = (unsigned long)cnt[0];
  if( sigs ) *sigs = (unsigned long)cnt[1];
  return 0;
}

extern "C" int
fdgpu_ed25519_fwide_count( fdgpu_ed25519_ctx_t * ctx, unsigned long * keys, unsigned long * sigs ) {
  if( keys ) *keys = 0UL;
  if( sigs ) *sigs = 0UL;
  if( !ctx || !ctx->half || !ctx->key_fixed || ctx->last_path != FDGPU_PATH_THROUGHPUT ) return 0;
  if( hipSetDevice( ctx->device ) != hipSuccess || hipStreamSynchronize( ctx->stream ) != hipSuccess ) return -1;
  u32 cnt[ 2 ] = { 0u, 0u };
  if( hipMemcpy( cnt, slow_word( ctx, FD_SW_HOT ) + FD_KC_FWK, sizeof(cnt), hipMemcpyDeviceToHost ) != hipSuccess ) return -1;
  if( keys ) *keys = (unsigned long)cnt[0];
  if( sigs ) *sigs = (unsigned long)cnt[1];
  return 0;
}

extern "C" int
fdgpu_ed25519_pinned_count( fdgpu_ed25519_ctx_t * ctx, unsigned long * keys, unsigned long * sigs ) {
  if( keys ) *keys = 0UL;
  if( sigs ) *sigs = 0UL;
  if( !ctx || !ctx->half || !ctx->key_fixed || ctx->last_path != FDGPU_PATH_THROUGHPUT ) return 0;
  if( hipSetDevice( ctx->device ) != hipSuccess || hipStreamSynchronize( ctx->stream ) != hipSuccess ) return -1;
  u32 cnt[ 2 ] = { 0u, 0u };
  if( hipMemcpy( cnt, slow_word( ctx, FD_SW_HOT ) + FD_KC_PINK, sizeof(cnt), hipMemcpyDeviceToHost ) != hipSuccess ) return -1;
  if( keys ) *keys = (unsigned long)cnt[0];
  if( sigs ) *sigs = (unsigned long)cnt[1];
  return 0;
}

extern "C" unsigned long
fdgpu_ed25519_pin_cap( fdgpu_ed25519_ctx_t * ctx ) {
  if( !ctx || !ctx->half || !ctx->key_fixed ) return 0UL;
  return fd_pin_list_cap( ctx->fb_cap );
}

/* Pinned keys.  The list is de-duplicated on the host (fd_pin_list.h); distinct key number j takes slot
   j.  Marking the cache dirty makes the next batch empty every slot before anything else (launch_half), after which
   its index lanes restore slots [0, npin): that is the emptying of every unpinned slot, and, should the build below
   fail, of the half-built ones too (npin is then 0).  The build: the keys into d_skey, fd_keypin_kernel (status,
   the 32 P_j), fd_ftab_kernel over all four groups of every slot, with its counters in words of d_Rxy, which no
   batch is using -- the batch's own counters stay the last batch's. */
extern "C" int
fdgpu_ed25519_set_pinned_keys( fdgpu_ed25519_ctx_t * ctx, unsigned char const * keys, unsigned long n,
                               unsigned char * status_out ) {
  if( !ctx || ( n && !keys ) ) { fd_err = "fdgpu_ed25519_set_pinned_keys: bad arguments"; return -1; }
  if( n > fdgpu_ed25519_pin_cap( ctx ) ) { fd_err = "fdgpu_ed25519_set_pinned_keys: more keys than fdgpu_ed25519_pin_cap"; return -1; }
  if( async_busy( ctx ) ) { fd_err = "fdgpu_ed25519_set_pinned_keys: the async pipeline holds a batch"; return -2; }
  if( ctx->fault ) { fd_err = "fdgpu_ed25519_set_pinned_keys: the context is faulted"; return -3; }
  if( !ctx->key_fixed ) return 0;                        /* (n = 0 on a context that cannot pin) */
  std::vector<unsigned int> slot_of( n ? n : 1UL ), first_of( n ? n : 1UL ), work( fd_pin_list_work( n ) );
  unsigned long m = fd_pin_list_dedup( keys, n, slot_of.data(), first_of.data(), work.data() );
  std::vector<unsigned char> uniq( 32UL * ( m ? m : 1UL ) ), st( m ? m : 1UL );
  for( unsigned long j=0UL; j<m; j++ ) memcpy( uniq.data() + 32UL*j, keys + 32UL*first_of[j], 32UL );
  HIPCHK( hipSetDevice( ctx->device ), -3 );
  HIPCHK( hipStreamSynchronize( ctx->stream ), -3 );
  ctx->npin = 0u; ctx->kc_dirty = 1;
  if( m ) {
    hipStream_t s = ctx->stream;
    u32 * pcnt = (u32 *)ctx->d_Rxy;
    HIPCHK( hipMemcpy( ctx->d_skey, uniq.data(), 32UL*m, hipMemcpyHostToDevice ), -3 );
    hipLaunchKernelGGL( fd_keypin_kernel, dim3( (unsigned)( ( (unsigned long)FD_FB_NT * m + FD_WG - 1UL ) / FD_WG ) ), dim3(FD_WG), 0, s,
                        (u32)m, (u32 const *)ctx->d_skey, ctx->d_sstat, ctx->d_fbase, ctx->d_flist, pcnt );
    /* (... and the wide tables of the pinned slots below wcap, their 16 extra base points first) */
    if( ctx->wcap )
      hipLaunchKernelGGL( fd_wbase_kernel, dim3( (unsigned)( ( 16UL * m + FD_WG - 1UL ) / FD_WG ) ), dim3(FD_WG), 0, s, (u32 const *)pcnt,
                          (u32 const *)ctx->d_flist, (unsigned char const *)ctx->d_sstat, (uint4 const *)ctx->d_fbase,
                          ctx->d_wbase, ctx->wcap );
    hipLaunchKernelGGL( fd_ftab_kernel, dim3( (unsigned)( ( ( ctx->wcap ? 28UL : 4UL ) * m + 1UL ) / 2UL ) ), dim3(FD_WG), 0, s,
                        (u32 const *)pcnt, (u32 const *)ctx->d_flist, (unsigned char const *)ctx->d_sstat,
                        (uint4 const *)ctx->d_fbase, ctx->d_ftab, 4u, (u32 const *)ctx->d_plist, 0u,
                        (uint4 const *)ctx->d_wbase, ctx->d_wtab, ctx->wcap, 1u );
    HIPCHK( hipGetLastError(), -3 );
    HIPCHK( hipStreamSynchronize( s ), -3 );
    HIPCHK( hipMemcpy( st.data(), ctx->d_sstat, m, hipMemcpyDeviceToHost ), -3 );
  }
  if( status_out ) for( unsigned long i=0UL; i<n; i++ ) status_out[i] = st[ slot_of[i] ];
  ctx->npin = (u32)m;
  return 0;
}

extern "C" unsigned long
fdgpu_ed25519_front_remaining( fdgpu_ed25519_ctx_t const * ctx ) {
  if( ctx->inflight.empty() ) return 0UL;
  fd_slot const & sl = ctx->slot[ ctx->inflight.front() ];
  return sl.txn_cnt - sl.cursor;
}

extern "C" int
fdgpu_ed25519_front_batch( fdgpu_ed25519_ctx_t const * ctx, unsigned long * txn_cnt, unsigned long * cursor, int * path ) {
  if( ctx->inflight.empty() ) { *txn_cnt = 0UL; *cursor = 0UL; *path = FDGPU_PATH_NONE; return 0; }
  fd_slot const & sl = ctx->slot[ ctx->inflight.front() ];
  *txn_cnt = sl.txn_cnt; *cursor = sl.cursor; *path = sl.path;
  return 1;
}

extern "C" void
fdgpu_ed25519_pipeline_state( fdgpu_ed25519_ctx_t const * ctx, unsigned long * filling, unsigned long * inflight ) {
  *filling  = ctx->slot[ ctx->cur ].state==0 ? ctx->slot[ ctx->cur ].txn_cnt : 0UL;
  *inflight = (unsigned long)ctx->inflight.size();
}

extern "C" unsigned long
fdgpu_ed25519_poll( fdgpu_ed25519_ctx_t * ctx, unsigned long * out_tags, signed char * out_codes,
                    unsigned long max, int blocking ) {
  return poll_any( ctx, out_tags, out_codes, NULL, NULL, NULL, max, blocking );
}

extern "C" unsigned long
fdgpu_ed25519_poll_raw( fdgpu_ed25519_ctx_t * ctx, unsigned long * out_tags, signed char * out_codes,
                        unsigned char * out_img, unsigned short * out_fp, unsigned long * out_dedup, unsigned long max,
                        int blocking ) {
  return poll_any( ctx, out_tags, out_codes, out_img, out_fp, out_dedup, max, blocking );
}

extern "C" void
fdgpu_ed25519_set_dedup( fdgpu_ed25519_ctx_t * ctx, int enable, unsigned long seed ) {
  ctx->dedup = enable ? 1 : 0; ctx->dedup_seed = seed;
}

extern "C" int
fdgpu_ed25519_set_dedup_seeds( fdgpu_ed25519_ctx_t * ctx, unsigned long const * seeds, int n ) {
  if( n < 0 || n > 16 || ( n && !seeds ) ) { fd_err = "fdgpu_ed25519_set_dedup_seeds: 0..16 seeds"; return -1; }
  /* element by element, with no transient zero: the verify service sets the seeds again when a tile attaches,
     and a launch thread may be copying them into a batch's kernel arguments meanwhile (launch_raw) -- the
     seeds of tiles already attached are rewritten with the same values */
  for( int i=0; i<16; i++ ) __atomic_store_n( &ctx->dedup_seeds[i], i < n ? seeds[i] : 0UL, __ATOMIC_RELAXED );
  __atomic_store_n( &ctx->dedup_nseed, n, __ATOMIC_RELEASE );
  ctx->dedup = 1;
  return 0;
}

extern "C" int
fdgpu_ed25519_set_record_fp_off( fdgpu_ed25519_ctx_t * ctx, int off ) {
  if( off < -1 || off > 253 ) { fd_err = "bad record footprint offset"; return -1; }
  ctx->rec_fp_off = off;
  return 0;
}

/* ---- drop-in synchronous API (fd_ed25519.h) ------------------------- */

static std::mutex g_mu;
static fdgpu_ed25519_ctx_t * g_ctx = NULL;

static int g_dropin_device = 0, g_dropin_semantics = FDGPU_SEMANTICS_AVX512;

static fdgpu_ed25519_ctx_t * global_ctx( void ) {
  if( g_ctx ) return g_ctx;
  g_ctx = fdgpu_ed25519_ctx_new( g_dropin_device, 64, 64, 1UL<<17, g_dropin_semantics );
  return g_ctx;
}

extern "C" int
fdgpu_ed25519_dropin_init( int device, int semantics ) {
  if( semantics!=FDGPU_SEMANTICS_AVX512 && semantics!=FDGPU_SEMANTICS_REF ) { fd_err = "bad semantics"; return -1; }
  std::lock_guard<std::mutex> lk( g_mu );
  if( g_ctx && ( g_ctx->device != device || g_ctx->semantics != semantics ) ) { fdgpu_ed25519_ctx_delete( g_ctx ); g_ctx = NULL; }
  g_dropin_device = device; g_dropin_semantics = semantics;
  return global_ctx() ? 0 : -2;
}

/* drop-in for messages whose descriptor would pass 64 KiB: digests first
   (fd_sha512_batch_kernel over n staged R_j||A_j||M copies), then the batch
   with an empty message and the digests in ctx->d_khash.  Returns the
   code, or 1 on a GPU error. */
static int
verify_long( fdgpu_ed25519_ctx_t * ctx, unsigned char const * msg, unsigned long msg_sz,
             unsigned char const * sigs, unsigned char const * pubs, unsigned long n ) {
  /* the batch SHA kernel takes 32-bit sizes: refuse before allocating anything */
  if( msg_sz > 0xffffffffUL - 64UL || n * ( 64UL + msg_sz ) > 0xffffffffUL ) { fd_err = "message too long"; return 1; }
  size_t one = 64UL + msg_sz, tot = n*one;
  std::vector<unsigned char> buf, dig;
  std::vector<unsigned long> off;
  std::vector<unsigned int>  hsz;
  try { buf.resize( tot ); off.resize( n ); hsz.resize( n ); dig.resize( 64*n ); }
  catch( std::bad_alloc const & ) { fd_err = "verify_long: out of host memory"; return 1; }
  for( unsigned long j=0; j<n; j++ ) {
    unsigned char * b = buf.data() + j*one;
    memcpy( b, sigs + 64*j, 32 ); memcpy( b + 32, pubs + 32*j, 32 );
    if( msg_sz ) memcpy( b + 64, msg, msg_sz );
    off[j] = j*one; hsz[j] = (unsigned)one;
  }
  if( fdgpu_sha512_batch_host( ctx->device, buf.data(), tot, off.data(), hsz.data(), n, dig.data() ) ) return 1;
  unsigned char pl[ 96*16 ];
  memcpy( pl, sigs, 64*n ); memcpy( pl + 64*n, pubs, 32*n );
  fdgpu_txn_desc_t d;
  d.payload_off = 0; d.sig_base = 0; d.payload_sz = (unsigned short)(96*n); d.message_off = (unsigned short)(96*n);
  d.acct_addr_off = (unsigned short)(64*n); d.signature_off = 0; d.sig_cnt = (unsigned char)n;
  if( hipSetDevice( ctx->device ) != hipSuccess || hipMalloc( (void **)&ctx->d_khash, 64*n ) != hipSuccess ) { fd_err = "hipMalloc"; return 1; }
  int rc = 1;
  signed char out = 0;
  if( hipMemcpy( ctx->d_khash, dig.data(), 64*n, hipMemcpyHostToDevice ) == hipSuccess &&
      !fdgpu_ed25519_verify_txns_host( ctx, pl, 96*n, &d, 1, &out, NULL ) ) rc = out;
  (void)hipFree( ctx->d_khash ); ctx->d_khash = NULL;
  return rc;
}

extern "C" int
fd_ed25519_verify_batch_single_msg( unsigned char const msg[], unsigned long const msg_sz,
                                    unsigned char const signatures[ 64 ], unsigned char const pubkeys[ 32 ],
                                    fd_sha512_t * shas[ 1 ], unsigned char const batch_sz ) {
  (void)shas;
  if( batch_sz==0 || batch_sz>16 ) return FD_ED25519_ERR_SIG;   /* fd_ed25519_user.c:238-241 */
  unsigned long n = batch_sz;
  unsigned long sz = 96UL*n + msg_sz;
  std::lock_guard<std::mutex> lk( g_mu );
  fdgpu_ed25519_ctx_t * ctx = global_ctx();
  if( !ctx ) { fprintf( stderr, "fdgpu: no GPU context: %s\n", fdgpu_last_error() ); abort(); }
  if( sz > 0xffffUL ) {
    /* beyond the 16-bit descriptor: k = SHA-512(R||A||M) by the batch SHA-512 kernel first, then the same
       verify with the digests handed in (same codes as the reference for any message length) */
    int r = verify_long( ctx, msg, msg_sz, signatures, pubkeys, n );
    if( r > 0 ) { fprintf( stderr, "fdgpu: verify failed: %s\n", fdgpu_last_error() ); abort(); }
    return r;
  }
  std::vector<unsigned char> buf( sz );
  memcpy( buf.data(), signatures, 64*n );
  memcpy( buf.data() + 64*n, pubkeys, 32*n );
  if( msg_sz ) memcpy( buf.data() + 96*n, msg, msg_sz );
  fdgpu_txn_desc_t d;
  d.payload_off = 0; d.sig_base = 0; d.payload_sz = (unsigned short)sz; d.message_off = (unsigned short)(96*n);
  d.acct_addr_off = (unsigned short)(64*n); d.signature_off = 0; d.sig_cnt = (unsigned char)n;
  signed char out = 0;
  if( fdgpu_ed25519_verify_txns_host( ctx, buf.data(), sz, &d, 1, &out, NULL ) ) {
    fprintf( stderr, "fdgpu: verify failed: %s\n", fdgpu_last_error() ); abort();
  }
  return out;
}

extern "C" int
fd_ed25519_verify( unsigned char const msg[], unsigned long msg_sz, unsigned char const sig[ 64 ],
                   unsigned char const public_key[ 32 ], fd_sha512_t * sha ) {
  fd_sha512_t * shas[1] = { sha };
  return fd_ed25519_verify_batch_single_msg( msg, msg_sz, sig, public_key, shas, 1 );
}

extern "C" char const *
fd_ed25519_strerror( int err ) {   /* fd_ed25519_user.c:312-322 */
  switch( err ) {
  case FD_ED25519_SUCCESS:    return "success";
  case FD_ED25519_ERR_SIG:    return "bad signature";
  case FD_ED25519_ERR_PUBKEY: return "bad public key";
  case FD_ED25519_ERR_MSG:    return "bad message";
  default: break;
  }
  return "unknown";
}
