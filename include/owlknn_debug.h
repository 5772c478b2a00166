/*
 * owlknn_debug.h -- a test hook on an engine's scratch memory (tknnDebugPoison), an entry point of libowl_mi355x.so on top of the
 * C ABI of owlknn.h.  Plain C99; link and load as owlknn.h says.  Nothing a product needs is in here.
 */
#pragma once
#include <stddef.h>

#include "owlknn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- poison: what one call leaves behind must not matter to the next ------------------------------------------------------------
 * Every call of an engine carves its scratch out of one workspace that only grows and is never cleared, and shares one block of
 * device counters, its host copy and a few lists with every other call.  A call is right only if every word it reads of them has
 * been written by that same call first ("State that carries from one call to the next", lists the exceptions).
 * tknnDebugPoison fills the parts named in `what` with `byte`, so that a test can show a call gives the same result whatever
 * was there:
 *   TKNN_POISON_WORKSPACE  the workspace, first grown to at least min_workspace_bytes (a fresh engine has none), all of it
 *   TKNN_POISON_COUNTERS   the device counters, all of them, and the whole of their pinned host copy
 *   TKNN_POISON_LISTS      the list of handed-over slots with its length, the list of tie slots, the halo pass's block masks and
 *                          cursors -- each as far as it is allocated
 *   TKNN_POISON_SOLVE      the per-slot solve state: done, intersections, next level, tie flags -- as far as allocated (at a
 *                          boundary between a phase-1 and a phase-2 solve this state is LIVE: do not poison it there)
 * `stream` is first made to wait for a DBSCAN side launch that no stream has waited for yet.  The device fills are asynchronous
 * fills on `stream`; the host copy is filled after the stream has been synchronised, so the call returns with everything done.
 * The trees, the batch layout, the boundary marks and every host flag are never touched.  *poisoned_bytes (optional): the bytes
 * filled, device and host together.
 * Errors, in this order: NULL engine: TKNN_E_ARG; a bit in `what` that no part has, byte outside 0 .. 255: TKNN_E_ARG.  A refused
 * call writes nothing. */
#define TKNN_POISON_WORKSPACE 1u
#define TKNN_POISON_COUNTERS 2u
#define TKNN_POISON_LISTS 4u
#define TKNN_POISON_SOLVE 8u
#define TKNN_POISON_ALL 15u
TKNN_API int tknnDebugPoison(tknnEngine e, unsigned what, int byte, size_t min_workspace_bytes, int64_t *poisoned_bytes, void *stream);

#ifdef __cplusplus
}
#endif
