#ifndef HEADER_fd_pin_list_h
#define HEADER_fd_pin_list_h

/* The host side of fdgpu_ed25519_set_pinned_keys' key list: the cap, and the de-duplication that
   gives every listed key its slot.  Plain C without a dependency, so that the engine (C++) and a stand-alone
   check program (fd_pin_list_check.c) compile the same text. */

#include <string.h>

/* The most keys a context with fb_cap slots can pin: the last quarter, the per-batch promotion bound, stays for
   the keys that batches find by themselves */
static inline unsigned long
fd_pin_list_cap( unsigned long fb_cap ) {
  return fb_cap - fb_cap / 4UL;
}

/* Words of work memory fd_pin_list_dedup needs for a list of n keys: an open-addressed table of a power of two of
   at least 2 n slots (0 = empty, else 1 + the slot of the key) */
static inline unsigned long
fd_pin_list_work( unsigned long n ) {
  unsigned long w = 4UL;
  while( w < 2UL * n ) w <<= 1;
  return w;
}

/* keys[32 n]: the list.  The distinct keys are numbered in the order of their first appearance: slot_of[i] (n
   entries) is the number of key i, first_of[j] (up to n entries) the list index at which key number j first
   appears.  work: fd_pin_list_work( n ) words.  Returns the count of distinct keys.  All 32 bytes are compared;
   the hash (FNV-1a) only orders the probes, and the table is never more than half full, so every probe
   sequence ends. */
static inline unsigned long
fd_pin_list_dedup( unsigned char const * keys, unsigned long n, unsigned int * slot_of, unsigned int * first_of,
                   unsigned int * work ) {
  unsigned long w = fd_pin_list_work( n ), m = 0UL;
  memset( work, 0, w * sizeof(unsigned int) );
  for( unsigned long i=0UL; i<n; i++ ) {
    unsigned char const * k = keys + 32UL * i;
    unsigned long h = 0xcbf29ce484222325UL;
    for( int b=0; b<32; b++ ) h = ( h ^ k[b] ) * 0x100000001b3UL;
    h ^= h >> 29;
    for( unsigned long p = h & ( w - 1UL );; p = ( p + 1UL ) & ( w - 1UL ) ) {
      unsigned int v = work[p];
      if( !v ) { work[p] = (unsigned int)m + 1U; first_of[m] = (unsigned int)i; slot_of[i] = (unsigned int)m; m++; break; }
      if( !memcmp( keys + 32UL * first_of[v - 1U], k, 32UL ) ) { slot_of[i] = v - 1U; break; }
    }
  }
  return m;
}

#endif /* HEADER_fd_pin_list_h */
