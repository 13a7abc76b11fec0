#ifndef HEADER_fd_shred_desc_h
#define HEADER_fd_shred_desc_h

/* Merkle shred descriptors (fdgpu_shred_desc_t): the rules that decide a record's code before any
   hashing, and where the hashing reads.  Plain C without a dependency, so that the engine's host code (C++), its
   kernels (HIP: FD_SHRED_DESC_FN adds __host__ __device__ there) and a stand-alone check program
   (fd_shred_desc_check.c) compile the same text.

   A shred is sz bytes at arena + off.  Its header fields lie in bytes [0x40, 0x59): fd_shred_fields reads them
   from the 7 little-endian 32-bit words that hold bytes [0x40, 0x5c), which the caller loads (the kernel with
   aligned dword loads and byte shifts, the host with memcpy); sz >= 88 makes all but the last three of those
   bytes the shred's own, and the last three decide nothing in a shred of 88 bytes (it fails sz < 1203 first).

   The first rule that fails decides the code, in this order (include/fd_ed25519_gpu.h has the values):

   descriptor  fd_shred_desc_bad: off + sz > arena_sz in 64 bits; key_idx neither FD_SHRED_NO_SIG nor below
               key_cnt; a signature wanted and sig_idx >= sig_cnt                             -> FD_SHRED_ERR_DESC
   parse       fd_shred_parse( shred, sz ) == NULL (src/ballet/shred/fd_shred.c), or a legacy variant 0xa5 /
               0x5a, which parses there and which every caller that derives a root rejects
               (src/disco/shred/fd_fec_resolver.c:360-363)                                     -> FD_SHRED_ERR_PARSE
   Merkle      fd_shred_merkle_root returns 0 on a fresh tree of 10 layers: depth >= 10 or leaf index > 511
               (src/ballet/bmtree/fd_bmtree.c:395-401); with FD_SHRED_STRICT_LEAF also leaf >= 2^depth, the
               resolver's own rule (fd_fec_resolver.c:412)                                     -> FD_SHRED_ERR_MERKLE

   Otherwise the leaf is SHA-256( 0x00 "SOLANA_MERKLE_SHREDS_LEAF" shred[64, moff) ), the proof's depth nodes of
   20 bytes start at shred + moff, and bit l of leaf says on which side of level l's merge the running node
   stands (0: left). */

#ifndef FD_SHRED_DESC_FN
#define FD_SHRED_DESC_FN static inline
#endif

#define FD_SHRED_NO_SIG      (0xFFFFU)   /* key_idx: derive the root only */
#define FD_SHRED_STRICT_LEAF (1U)        /* flags: leaf < 2^depth as well */
#define FD_SHRED_ERR_DESC    (-18)
#define FD_SHRED_ERR_PARSE   (-19)
#define FD_SHRED_ERR_MERKLE  (-20)

#define FD_SHRED_HDR_SZ      (88U)       /* min( data header, code header ): fd_shred_parse's first bound */
#define FD_SHRED_DATA_SZ     (1203U)     /* FD_SHRED_MIN_SZ: a data shred, its proof included */
#define FD_SHRED_CODE_SZ     (1228U)     /* FD_SHRED_MAX_SZ: a code shred */
#define FD_SHRED_NODE_SZ     (20U)       /* a proof node */
#define FD_SHRED_DEPTH_MAX   (10U)       /* layers of the reference's tree: depth < 10 */
#define FD_SHRED_LEAF_MAX    (511U)
#define FD_SHRED_FIELD_WORDS (7)         /* words at shred + 0x40 that fd_shred_fields reads */

typedef struct fd_shred_fields {
  unsigned char  variant;       /* 0x40 */
  unsigned long  slot;          /* 0x41 */
  unsigned int   idx;           /* 0x49 */
  unsigned int   fec_set_idx;   /* 0x4f */
  unsigned short h53;           /* 0x53  data: parent_off   code: data_cnt */
  unsigned char  flags;         /* 0x55  data: flags */
  unsigned short h55;           /* 0x55                     code: code_cnt */
  unsigned short size;          /* 0x56  data: size */
  unsigned short h57;           /* 0x57                     code: idx */
} fd_shred_fields_t;

typedef struct fd_shred_info {
  unsigned int leaf;            /* the shred's index in its FEC set's tree */
  unsigned int depth;           /* proof nodes */
  unsigned int moff;            /* the Merkle-protected bytes are shred[64, moff); the proof starts at moff */
} fd_shred_info_t;

/* byte j of the little-endian words w */
FD_SHRED_DESC_FN unsigned int
fd_shred_byte( unsigned int const * w, unsigned int j ) { return ( w[ j >> 2 ] >> ( 8U * ( j & 3U ) ) ) & 0xFFU; }

/* the header fields from w[k] = bytes [0x40 + 4k, 0x44 + 4k) of the shred, little endian, k < 7 */
FD_SHRED_DESC_FN void
fd_shred_fields( unsigned int const * w, fd_shred_fields_t * f ) {
  /* (no loop and no run-time index: in a kernel w stays in registers) */
  unsigned int lo = ( w[0] >> 8 ) | ( w[1] << 24 ), hi = ( w[1] >> 8 ) | ( w[2] << 24 );
  f->variant     = (unsigned char)fd_shred_byte( w, 0U );
  f->slot        = (unsigned long)lo | ( (unsigned long)hi << 32 );
  f->idx         = fd_shred_byte( w,  9U ) | ( fd_shred_byte( w, 10U ) << 8 ) | ( fd_shred_byte( w, 11U ) << 16 ) | ( fd_shred_byte( w, 12U ) << 24 );
  f->fec_set_idx = fd_shred_byte( w, 15U ) | ( fd_shred_byte( w, 16U ) << 8 ) | ( fd_shred_byte( w, 17U ) << 16 ) | ( fd_shred_byte( w, 18U ) << 24 );
  f->h53         = (unsigned short)( fd_shred_byte( w, 19U ) | ( fd_shred_byte( w, 20U ) << 8 ) );
  f->flags       = (unsigned char)fd_shred_byte( w, 21U );
  f->h55         = (unsigned short)( fd_shred_byte( w, 21U ) | ( fd_shred_byte( w, 22U ) << 8 ) );
  f->size        = (unsigned short)( fd_shred_byte( w, 22U ) | ( fd_shred_byte( w, 23U ) << 8 ) );
  f->h57         = (unsigned short)( fd_shred_byte( w, 23U ) | ( fd_shred_byte( w, 24U ) << 8 ) );
}

/* 1 if the descriptor is bad.  The sum in 64 bits: an offset near 2^32 does not wrap. */
FD_SHRED_DESC_FN int
fd_shred_desc_bad( unsigned int off, unsigned int sz, unsigned int key_idx, unsigned int sig_idx,
                   unsigned long arena_sz, unsigned long key_cnt, unsigned long sig_cnt ) {
  int want_sig = key_idx != FD_SHRED_NO_SIG;
  return ( (unsigned long)off + (unsigned long)sz > arena_sz )
       | ( want_sig & ( (unsigned long)key_idx >= key_cnt ) )
       | ( want_sig & ( (unsigned long)sig_idx >= sig_cnt ) );
}

/* type bits of a variant */
FD_SHRED_DESC_FN int fd_shred_is_data( unsigned int type )     { return ( type == 0x80U ) | ( type == 0x90U ) | ( type == 0xb0U ); }
FD_SHRED_DESC_FN int fd_shred_is_code( unsigned int type )     { return ( type == 0x40U ) | ( type == 0x60U ) | ( type == 0x70U ); }
FD_SHRED_DESC_FN int fd_shred_is_chained( unsigned int type )  { return ( type == 0x90U ) | ( type == 0x60U ) | ( type == 0xb0U ) | ( type == 0x70U ); }
FD_SHRED_DESC_FN int fd_shred_is_resigned( unsigned int type ) { return ( type == 0xb0U ) | ( type == 0x70U ); }

/* 0 and *info, or FD_SHRED_ERR_PARSE / FD_SHRED_ERR_MERKLE, for a shred of sz >= FD_SHRED_HDR_SZ bytes with
   header fields f; FD_SHRED_ERR_PARSE for a shorter one, whose fields are not looked at (f may then hold
   anything).  flags: the descriptor's. */
FD_SHRED_DESC_FN int
fd_shred_classify( fd_shred_fields_t const * f, unsigned int sz, unsigned int flags, fd_shred_info_t * info ) {
  info->leaf = 0U; info->depth = 0U; info->moff = 0U;
  if( sz < FD_SHRED_HDR_SZ ) return FD_SHRED_ERR_PARSE;
  unsigned int type = (unsigned int)f->variant & 0xf0U, d = (unsigned int)f->variant & 0xfU;
  int data = fd_shred_is_data( type ), code = fd_shred_is_code( type );
  if( !( data | code ) ) return FD_SHRED_ERR_PARSE;                       /* legacy 0xa5 / 0x5a included */
  unsigned int chained = (unsigned int)fd_shred_is_chained( type ), resigned = (unsigned int)fd_shred_is_resigned( type );
  unsigned int trailer = FD_SHRED_NODE_SZ * d + 32U * chained + 64U * resigned;
  unsigned int full    = data ? FD_SHRED_DATA_SZ : FD_SHRED_CODE_SZ;
  unsigned int leaf;
  if( data ) {
    unsigned long parent_off = (unsigned long)f->h53;
    if( (unsigned int)f->size < FD_SHRED_HDR_SZ )               return FD_SHRED_ERR_PARSE;
    if( sz < FD_SHRED_DATA_SZ )                                 return FD_SHRED_ERR_PARSE;
    if( (unsigned int)f->size + trailer > FD_SHRED_DATA_SZ )    return FD_SHRED_ERR_PARSE;
    if( ( (unsigned int)f->flags & 0xC0U ) == 0x80U )           return FD_SHRED_ERR_PARSE;
    if( parent_off > f->slot )                                  return FD_SHRED_ERR_PARSE;
    if( ( f->slot != 0UL ) & ( parent_off == 0UL ) )            return FD_SHRED_ERR_PARSE;
    if( ( f->slot > 1UL ) & ( parent_off == f->slot ) )         return FD_SHRED_ERR_PARSE;
    if( f->idx < f->fec_set_idx )                               return FD_SHRED_ERR_PARSE;
    leaf = f->idx - f->fec_set_idx;
  } else {
    unsigned int data_cnt = f->h53, code_cnt = f->h55, cidx = f->h57;
    if( sz < FD_SHRED_CODE_SZ )                                 return FD_SHRED_ERR_PARSE;
    if( cidx >= code_cnt )                                      return FD_SHRED_ERR_PARSE;
    if( cidx > f->idx )                                         return FD_SHRED_ERR_PARSE;
    if( ( data_cnt == 0U ) | ( code_cnt == 0U ) )               return FD_SHRED_ERR_PARSE;
    if( code_cnt > 256U )                                       return FD_SHRED_ERR_PARSE;
    if( data_cnt + code_cnt > 256U )                            return FD_SHRED_ERR_PARSE;
    leaf = cidx + data_cnt;
  }
  if( d >= FD_SHRED_DEPTH_MAX )                                 return FD_SHRED_ERR_MERKLE;
  if( leaf > FD_SHRED_LEAF_MAX )                                return FD_SHRED_ERR_MERKLE;
  if( ( flags & FD_SHRED_STRICT_LEAF ) && leaf >= ( 1U << d ) ) return FD_SHRED_ERR_MERKLE;
  info->leaf  = leaf;
  info->depth = d;
  info->moff  = full - FD_SHRED_NODE_SZ * d - 64U * resigned;
  return 0;
}

#endif /* HEADER_fd_shred_desc_h */
