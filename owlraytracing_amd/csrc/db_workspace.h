// db_workspace.h -- RT-DBSCAN's scratch (db_call.h, dbscan.hip) as byte offsets into the engine's workspace: one layout for the full
// clustering (tknnDbscan, tknnDbscanAssign), one for a growth round (tknnDbscanNoise, the rounds of tknnDbscanAuto), one for
// the labels of points that are not in the set (tknnDbscanQuery).  The
// offsets are computed here and nowhere else; no HIP in this file (tests/test_db_workspace.py compiles it for the host).
// n: points of the tree, one sorted slot each; m: query points of tknnDbscanQuery.  Words are int32.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace owlmi {

constexpr int kDbBlock = 256;  // slots per workgroup of the kernels that stream over the slots
// every region begins at a multiple of this: the kernels move four consecutive slots' words as one 16-byte load or store
// (db_flatten_kernel, db_label_kernel into by_slot) whatever n is
constexpr size_t kDbRegionAlign = 16;
// what follows a layout in the workspace (the library scan's temporary storage) begins at a multiple of this
constexpr size_t kDbScanAlign = 256;
constexpr size_t db_round_up(size_t bytes, size_t to) { return (bytes + to - 1) / to * to; }
// two words per workgroup of kDbBlock slots -- its count of something, then its place among all of them -- and room to spare
constexpr size_t db_block_places_bytes(size_t n) { return db_round_up((n / kDbBlock + 2) * 8, kDbRegionAlign); }

template <class T>
T *db_at(void *workspace, size_t offset) { return reinterpret_cast<T *>(static_cast<char *>(workspace) + offset); }
// hands out consecutive regions
struct DbCarver {
  size_t end = 0;
  size_t take(size_t bytes) { return (end = db_round_up(end + bytes, kDbRegionAlign)) - db_round_up(bytes, kDbRegionAlign); }
};

// The full clustering.  Launch order: core flags, next_core, [border walk on the side stream], group list, union pass 1,
// uniform, union pass 2, flatten, root, scan, labels, rows.
struct DbClusterWs {
  size_t parent;        // n words: union-find over slots; core-flag kernel .. label kernel
  // n words under three names, one after the other:
  //   groups   the list of groups that have a core point; db_group_list_kernel .. the last union launch
  //   is_root  zeroed by db_flatten_kernel, set by db_root_kernel at each cluster's smallest row, summed into `rank`
  //   by_slot  labels by slot; db_label_kernel .. db_rows_from_slots_kernel
  size_t roots;
  // n + 1 words under four names, one after the other:
  //   pos       slot of the r-th core point (+ a sentinel); db_core_pos_blocks_kernel .. db_next_core_blocks_kernel
  //   group_at  per slot, the group it leads or LBVH_END; db_group_kernel .. db_group_list_kernel
  //   uni_leaf  per slot, the set of a listed single-point group; db_uniform_kernel .. the second union launch
  //   rank      per row, the cluster numbered from that row (exclusive sum of is_root) .. db_label_kernel
  size_t ranks;
  size_t next_core;     // n + 1 words: first core slot at or after a slot; db_next_core_blocks_kernel .. label kernel
  size_t core_sorted;   // n bytes: core flag per slot; core-flag kernel .. label kernel
  size_t min_row;       // n words: at roots, the cluster's smallest row; filled by db_group_kernel (per-point unions: a memset
                        // after them), lowered by db_flatten_kernel .. label kernel
  size_t not_core;      // n words: the slots that are not core, in slot order; db_core_pos_blocks_kernel .. label kernel
  size_t border_lists;  // n words: per listed slot a count and its core neighbours; db_border_walk_kernel .. label kernel
  size_t uni;           // n words: per tree node, the one set below it; filled by db_group_kernel, db_uniform_kernel .. the
                        // second union launch
  size_t block_places;  // db_block_places_bytes(n): core slots per workgroup and their sums; then listed groups likewise
  size_t pk_diag;       // diagnostic library only: 16 bytes per packet of db_group_union_kernel (zero bytes otherwise)
  size_t end;

  size_t groups() const { return roots; }
  size_t is_root() const { return roots; }
  size_t by_slot() const { return roots; }
  size_t pos() const { return ranks; }
  size_t group_at() const { return ranks; }
  size_t uni_leaf() const { return ranks; }
  size_t rank() const { return ranks; }

  static size_t max_packets(size_t n) { return n / 64 + 1; }
  static DbClusterWs of(size_t n, bool diag_records) {
    DbCarver c;
    DbClusterWs w;
    w.parent = c.take(n * 4), w.roots = c.take(n * 4), w.ranks = c.take((n + 1) * 4), w.next_core = c.take((n + 1) * 4);
    w.core_sorted = c.take(n), w.min_row = c.take(n * 4), w.not_core = c.take(n * 4), w.border_lists = c.take(n * 4);
    w.uni = c.take(n * 4), w.block_places = c.take(db_block_places_bytes(n));
    w.pk_diag = c.take(diag_records ? max_packets(n) * 16 : 0), w.end = c.end;
    return w;
  }
  static size_t bytes(size_t n, bool diag_records) { return of(n, diag_records).end; }
};

// A growth round: core flags, next_core, noise probe.  Nothing is shared: every region has one name for the whole round,
// and core_sorted and noise live from round to round of tknnDbscanAuto.
struct DbProbeWs {
  size_t near_node;     // n words: where a slot's noise probe starts; core-flag kernel .. noise probe
  size_t pos;           // n + 1 words: slot of the r-th core point (+ a sentinel)
  size_t next_core;     // n + 1 words
  size_t block_places;  // db_block_places_bytes(n): core slots per workgroup and their sums
  size_t core_sorted;   // n bytes: core flag per slot (a later round keeps the flags of the rounds before)
  size_t noise;         // n bytes: per slot, 1 = noise in this round
  size_t end;

  static DbProbeWs of(size_t n) {
    DbCarver c;
    DbProbeWs w;
    w.near_node = c.take(n * 4), w.pos = c.take((n + 1) * 4), w.next_core = c.take((n + 1) * 4);
    w.block_places = c.take(db_block_places_bytes(n)), w.core_sorted = c.take(n), w.noise = c.take(n), w.end = c.end;
    return w;
  }
  static size_t bytes(size_t n) { return of(n).end; }
};

// Labels for m points that are not in the set: core flags from the caller's labels, next_core, the queries' order along the
// tree's curve (query_order.h), one traversal.  Nothing is shared.  The library's temporary storage (the sum over the
// workgroups' counts, then the sort of the queries: one after the other, so the larger of the two) follows the layout as
// it follows the others.
struct DbQueryWs {
  size_t pos;           // n + 1 words: slot of the r-th core point (+ a sentinel)
  size_t next_core;     // n + 1 words
  size_t block_places;  // db_block_places_bytes(n): core slots per workgroup and their sums
  size_t core_sorted;   // n bytes: core flag per slot
  size_t codes;         // m words: the queries' curve keys, caller order; query_code_kernel .. the sort
  size_t codes_sorted;  // m words: the sort's other key column
  size_t order_in;      // m words: 0 .. m - 1; query_code_kernel .. the sort
  size_t order;         // m words: the caller's index of the query at each sorted position; the sort .. db_query_kernel
  size_t end;

  static DbQueryWs of(size_t n, size_t m) {
    DbCarver c;
    DbQueryWs w;
    w.pos = c.take((n + 1) * 4), w.next_core = c.take((n + 1) * 4), w.block_places = c.take(db_block_places_bytes(n));
    w.core_sorted = c.take(n), w.codes = c.take(m * 4), w.codes_sorted = c.take(m * 4), w.order_in = c.take(m * 4);
    w.order = c.take(m * 4), w.end = c.end;
    return w;
  }
  static size_t bytes(size_t n, size_t m) { return of(n, m).end; }
};

}  // namespace owlmi
