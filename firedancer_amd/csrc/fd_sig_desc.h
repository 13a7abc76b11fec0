#ifndef HEADER_fd_sig_desc_h
#define HEADER_fd_sig_desc_h

/* Per-signature descriptors (fdgpu_sig_desc_t): the validity test, the packed size of a record and the
   rule that places the records of a batch in the pack arena.  Plain C without a dependency, so that the engine's
   host code (C++), its kernels (HIP: FD_SIG_DESC_FN adds __host__ __device__ there) and a stand-alone check
   program (fd_sig_desc_check.c) compile the same text.

   A record is one (signature, public key, message) triple named by four 32-bit byte offsets into an arena of
   arena_sz bytes.  Packed, it is the one-signer transaction sig(64) | pub(32) | msg(msg_sz), padded with zero
   bytes to a multiple of 8 (what fdgpu_ed25519_verify_many_host's staging writes).

   A bad descriptor -- a range that leaves the arena, or a message over FD_SIG_DESC_MSG_MAX -- is flagged
   (FD_SIG_DESC_BAD) and still takes a place: 96 zero bytes with an empty message.  So record i is transaction
   i and signature i of the batch, and neither needs a second scan.  The verify kernels see that place as one
   signature of the all-zero public key over an empty message, and the diagnostic counters (key_count, hot_count,
   ...) count it so; its code is replaced by FDGPU_ERR_DESC behind the batch.

   Capacity.  off[i] is the exclusive prefix sum of the sizes, and a record whose end off[i] + sz[i] passes the
   capacity cap is flagged (FD_SIG_DESC_OVER) and not copied.  Every record behind it is flagged too, and that is
   no extra rule: a flagged record still has a size of at least 96, so the prefix sum is strictly monotone and
   every later record also ends past cap.  The records [0, k) that fit are exactly those of a batch cut at k. */

#ifndef FD_SIG_DESC_FN
#define FD_SIG_DESC_FN static inline
#endif

#define FD_SIG_DESC_MSG_MAX (65439UL)   /* FDGPU_MSG_MAX: 96 + msg_sz fits the 16-bit payload_sz */
#define FD_SIG_DESC_HDR     (96U)       /* sig | pub */
#define FD_SIG_DESC_BAD     (1)         /* flag bit: the descriptor names bytes outside the arena or too long a message */
#define FD_SIG_DESC_OVER    (2)         /* flag bit: the record's packed end passes the capacity */

/* 1 if the descriptor is bad.  All sums in 64 bits: an offset near 2^32 does not wrap. */
FD_SIG_DESC_FN int
fd_sig_desc_bad( unsigned int sig_off, unsigned int pub_off, unsigned int msg_off, unsigned int msg_sz,
                 unsigned long arena_sz ) {
  return ( (unsigned long)sig_off + 64UL > arena_sz ) | ( (unsigned long)pub_off + 32UL > arena_sz )
       | ( (unsigned long)msg_off + (unsigned long)msg_sz > arena_sz ) | ( (unsigned long)msg_sz > FD_SIG_DESC_MSG_MAX );
}

/* The record's packed size: 96 + msg_sz rounded up to 8, or 96 for a bad one (*bad = 1).  At most 65,536. */
FD_SIG_DESC_FN unsigned int
fd_sig_desc_size( unsigned int sig_off, unsigned int pub_off, unsigned int msg_off, unsigned int msg_sz,
                  unsigned long arena_sz, int * bad ) {
  int b = fd_sig_desc_bad( sig_off, pub_off, msg_off, msg_sz, arena_sz );
  *bad = b;
  return b ? FD_SIG_DESC_HDR : ( FD_SIG_DESC_HDR + msg_sz + 7U ) & ~7U;
}

/* 1 if a record of sz bytes at offset off of the pack arena ends past cap */
FD_SIG_DESC_FN int
fd_sig_desc_over( unsigned long off, unsigned int sz, unsigned long cap ) {
  return off + (unsigned long)sz > cap;
}

/* Host reference of the whole placement (what the size, scan and place kernels compute together), over
   descriptors given as cnt x 4 words { sig_off, pub_off, msg_off, msg_sz }: off[i], flag[i] (FD_SIG_DESC_BAD |
   FD_SIG_DESC_OVER; off[i] of a record flagged OVER is where it would have started).  Returns the records in
   front of the first one flagged OVER (cnt if none): those that were copied. */
FD_SIG_DESC_FN unsigned long
fd_sig_desc_place( unsigned int const * desc, unsigned long cnt, unsigned long arena_sz, unsigned long cap,
                   unsigned long * off, unsigned char * flag ) {
  unsigned long at = 0UL, fit = cnt;
  for( unsigned long i=0UL; i<cnt; i++ ) {
    int bad;
    unsigned int sz = fd_sig_desc_size( desc[4UL*i], desc[4UL*i+1UL], desc[4UL*i+2UL], desc[4UL*i+3UL], arena_sz, &bad );
    int over = fd_sig_desc_over( at, sz, cap );
    if( over && fit == cnt ) fit = i;
    off[i]  = at;
    flag[i] = (unsigned char)( ( bad ? FD_SIG_DESC_BAD : 0 ) | ( over ? FD_SIG_DESC_OVER : 0 ) );
    at += (unsigned long)sz;
  }
  return fit;
}

#endif /* HEADER_fd_sig_desc_h */
