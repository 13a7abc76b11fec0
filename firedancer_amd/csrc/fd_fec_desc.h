#ifndef HEADER_fd_fec_desc_h
#define HEADER_fd_fec_desc_h

/* FEC sets (fdgpu_fec_desc_t / fdgpu_fec_member_t): the shape of a set's Merkle tree and the rules that
   decide a set's code before any hashing.  Plain C on top of fd_shred_desc.h, so that the engine's host code, its
   kernel (fd_fec_tree_kernel) and a stand-alone check program (fd_fec_desc_check.c) compile the same text.

   The tree over n leaves (src/ballet/bmtree/fd_bmtree.c, restated): layer 0 is the leaves, layer l + 1 node j is
   the merge of layer l's nodes 2j and 2j + 1, the last node of an odd layer merged with itself.  Layer l has
   ceil( n / 2^l ) nodes; the root is the one node of layer D, D = 0 for n = 1 and floor( log2( n - 1 ) ) + 1
   otherwise.  Leaf j's proof node at layer l < D is node ( j >> l ) ^ 1 of layer l, or node j >> l itself where
   that index is past the layer's end.

   A set's leaves are members [member0, member0 + cnt) of the member array, in tree order; member j's shred lies at
   arena + off.  The first rule that fails decides the set's code:

   descriptor  fd_fec_set_bad (cnt, the member range, the key and the slot) or, for some member,
               fd_fec_range_bad: off + 1203 > arena_sz, or -- the variant byte is read only once that holds -- a
               code shred with off + 1228 > arena_sz                                         -> FD_SHRED_ERR_DESC
   member      fd_fec_member_bad for some member j: the shred does not classify (STRICT_LEAF) as leaf j at depth D,
               or disagrees with member 0 (slot, version, fec_set_idx, type up to data / code, parent_off among
               data, data_cnt / code_cnt among code with their sum cnt); fd_fec_words_differ on the chained root
               or the signature                                                              -> FD_FEC_ERR_MEMBER
   root        FD_FEC_CHECK_ROOT and the tree's root is not the expected one                 -> FD_FEC_ERR_ROOT
   proof       FD_FEC_CHECK_PROOFS and a member without FD_FEC_FILL carries other bytes than the tree's
                                                                                             -> FD_FEC_ERR_PROOF */

#include "fd_shred_desc.h"

#define FD_FEC_ERR_MEMBER   (-21)
#define FD_FEC_ERR_ROOT     (-22)
#define FD_FEC_ERR_PROOF    (-23)
#define FD_FEC_LEAF_MAX     (256U)
#define FD_FEC_FILL         (1U)
#define FD_FEC_CHECK_ROOT   (1U)
#define FD_FEC_CHECK_PROOFS (2U)

/* layers under the root of a tree of n >= 1 leaves */
FD_SHRED_DESC_FN unsigned int
fd_fec_depth( unsigned int n ) {
  unsigned int d = 0U;
  while( ( 1U << d ) < n ) d++;
  return d;
}

/* nodes of layer l */
FD_SHRED_DESC_FN unsigned int
fd_fec_layer_cnt( unsigned int n, unsigned int l ) { return ( n + ( 1U << l ) - 1U ) >> l; }

/* nodes that the layers under the root hold, for any n <= lanes (a multiple of 64): a bound, 2 n + D at most */
FD_SHRED_DESC_FN unsigned int
fd_fec_node_cap( unsigned int lanes ) { return 2U * lanes + 8U; }

/* index inside layer l of leaf j's proof node */
FD_SHRED_DESC_FN unsigned int
fd_fec_sibling( unsigned int j, unsigned int l, unsigned int n ) {
  unsigned int s = ( j >> l ) ^ 1U;
  return s < fd_fec_layer_cnt( n, l ) ? s : ( j >> l );
}

/* 1 if the set's descriptor is bad.  The sum in 64 bits. */
FD_SHRED_DESC_FN int
fd_fec_set_bad( unsigned int member0, unsigned int cnt, unsigned int key_idx, unsigned int sig_idx,
                unsigned long member_cnt, unsigned long key_cnt, unsigned long sig_cnt ) {
  int want_sig = key_idx != FD_SHRED_NO_SIG;
  return ( cnt == 0U ) | ( cnt > FD_FEC_LEAF_MAX )
       | ( (unsigned long)member0 + (unsigned long)cnt > member_cnt )
       | ( want_sig & ( (unsigned long)key_idx >= key_cnt ) )
       | ( want_sig & ( (unsigned long)sig_idx >= sig_cnt ) );
}

/* 1 if a member's shred cannot be looked at: call it first with have_variant = 0 (variant is then ignored), and,
   if that gives 0, with the byte at off + 0x40 */
FD_SHRED_DESC_FN int
fd_fec_range_bad( unsigned int off, unsigned long arena_sz, int have_variant, unsigned int variant ) {
  if( (unsigned long)off + (unsigned long)FD_SHRED_DATA_SZ > arena_sz ) return 1;
  if( !have_variant ) return 0;
  return fd_shred_is_code( variant & 0xf0U ) & ( (unsigned long)off + (unsigned long)FD_SHRED_CODE_SZ > arena_sz );
}

/* the shred version (bytes 0x4d, 0x4e) from the words fd_shred_fields reads */
FD_SHRED_DESC_FN unsigned int
fd_fec_version( unsigned int const * w ) { return fd_shred_byte( w, 13U ) | ( fd_shred_byte( w, 14U ) << 8 ); }

/* the type of the other kind that goes with a type: Merkle, chained and resigned pair up */
FD_SHRED_DESC_FN unsigned int
fd_fec_type_mate( unsigned int type ) {
  switch( type ) {
  case 0x80U: return 0x40U;  case 0x40U: return 0x80U;
  case 0x90U: return 0x60U;  case 0x60U: return 0x90U;
  case 0xb0U: return 0x70U;  case 0x70U: return 0xb0U;
  default:    return 0x100U;                                  /* (no type) */
  }
}

/* 1 if member j of a set of cnt leaves breaks a rule that its header fields decide: f / ver are its fields and
   version, f0 / ver0 member 0's, fc the fields of the set's first code member (looked at only if this one is a
   code shred, which then exists).  *info is the member's, valid if 0 is returned. */
FD_SHRED_DESC_FN int
fd_fec_member_bad( fd_shred_fields_t const * f, unsigned int ver, fd_shred_fields_t const * f0, unsigned int ver0,
                   fd_shred_fields_t const * fc, unsigned int j, unsigned int cnt, fd_shred_info_t * info ) {
  unsigned int type = (unsigned int)f->variant & 0xf0U, type0 = (unsigned int)f0->variant & 0xf0U;
  unsigned int sz   = fd_shred_is_code( type ) ? FD_SHRED_CODE_SZ : FD_SHRED_DATA_SZ;
  if( fd_shred_classify( f, sz, FD_SHRED_STRICT_LEAF, info ) )  return 1;
  if( info->depth != fd_fec_depth( cnt ) )                      return 1;
  if( info->leaf != j )                                         return 1;
  if( f->slot != f0->slot )                                     return 1;
  if( ver != ver0 )                                             return 1;
  if( f->fec_set_idx != f0->fec_set_idx )                       return 1;
  if( ( type != type0 ) & ( type != fd_fec_type_mate( type0 ) ) ) return 1;
  if( fd_shred_is_data( type ) ) {
    /* member 0 is the first data member: as leaf 0 it cannot be a code shred, whose leaf is code.idx + data_cnt
       with data_cnt >= 1; if it is one, it fails its own leaf rule and the set with it */
    if( fd_shred_is_data( type0 ) & ( f->h53 != f0->h53 ) )     return 1;
  } else {
    if( (unsigned int)f->h53 + (unsigned int)f->h55 != cnt )    return 1;
    if( ( f->h53 != fc->h53 ) | ( f->h55 != fc->h55 ) )         return 1;
  }
  return 0;
}

/* 1 if two runs of n words differ */
FD_SHRED_DESC_FN int
fd_fec_words_differ( unsigned int const * a, unsigned int const * b, unsigned int n ) {
  unsigned int x = 0U;
  for( unsigned int k=0U; k<n; k++ ) x |= a[k] ^ b[k];
  return x != 0U;
}

#endif /* HEADER_fd_fec_desc_h */
