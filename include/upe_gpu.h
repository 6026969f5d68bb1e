/*
 * upe_gpu.h — C ABI of the MI355X batch dataplane for UPE's per-packet worker hot path.
 *
 * This is the drop-in boundary.  The reference runs the path one packet at a
 * time inside process_packet() (reference src/worker.c:106-253): parse_flow_key()
 * (src/parser.c:6-111) -> rule_table_match() (src/rule_table.c:163-176) -> counters and
 * rule_stats (src/worker.c:119-153) -> L3 forward rewrite with the one-entry L1 neighbour caches
 * and arp_get_mac()/ndp_get_mac() (src/worker.c:155-244, src/arp_table.c:55-80,
 * src/ndp_table.c:67-86).  This library runs the same semantics over a whole batch of packets
 * resident in GPU memory with one HIP kernel, bit-exact per packet.
 *
 * The reference surface is kept as plain data: every struct below is an ABI mirror of the
 * reference layout (same size, same offsets, checked by _Static_assert), so a C caller passes
 * rt->rules / arpt->entries / ndpt->entries / tx->eth_addr straight through without conversion.
 *
 * Conventions follow the reference (SURVEY.md §8(b) "Errors"): int 0 on success / -1 on failure,
 * NULL for a failed constructor, and upe_gpu_last_error() for a message (thread-local).  No C++
 * exception crosses this ABI.  A context is owned by one worker thread (one HIP stream); it is
 * not internally locked, exactly like a reference worker_t.
 */
#ifndef UPE_GPU_H
#define UPE_GPU_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------ */
/* ABI mirrors of the reference layouts                                                        */
/* ------------------------------------------------------------------------------------------ */

/* Mirrors ip_addr_t, reference include/parser.h:129-132.  IPv4 is host order in .v4 (ntohl),
 * IPv6 is wire-order bytes. */
typedef union {
    uint32_t v4;
    uint8_t v6[16];
} upe_ip_addr_t;

/* Mirrors flow_key_t, reference include/parser.h:134-141 (44 bytes). */
typedef struct {
    uint8_t ip_ver;
    upe_ip_addr_t src_ip;
    upe_ip_addr_t dst_ip;
    uint16_t src_port;
    uint16_t dst_port;
    uint8_t protocol;
} upe_flow_key_t;

/* Mirrors action_type_t / flow_action_t, reference include/rule_table.h:9-17. */
enum { UPE_ACT_DROP = 0, UPE_ACT_FWD = 1 };
typedef struct {
    int32_t type;        /* action_type_t is an int-sized enum */
    int32_t out_ifindex; /* never read by the worker (all TX goes to tx->ifindex) */
} upe_flow_action_t;

/* Mirrors rule_t, reference include/rule_table.h:19-35 (92 bytes). */
typedef struct {
    uint32_t priority;
    uint8_t ip_ver;
    upe_ip_addr_t src_ip;
    upe_ip_addr_t src_mask;
    upe_ip_addr_t dst_ip;
    upe_ip_addr_t dst_mask;
    uint16_t src_port;
    uint16_t dst_port;
    uint8_t protocol;
    upe_flow_action_t action;
    uint32_t rule_id;
} upe_rule_t;

/* Mirrors arp_entry_t, reference include/arp_table.h:13-18 (32 bytes on LP64). */
typedef struct {
    uint32_t ip;
    uint8_t mac[6];
    int64_t update_at; /* time_t */
    bool valid;
} upe_arp_entry_t;

/* Mirrors ndp_entry_t, reference include/ndp_table.h:13-18 (40 bytes on LP64). */
typedef struct {
    uint8_t ip[16];
    uint8_t mac[6];
    int64_t update_at; /* time_t */
    bool valid;
} upe_ndp_entry_t;

/* Mirrors rule_stat_t, reference include/worker.h:18-21. */
typedef struct {
    uint64_t packets;
    uint64_t bytes;
} upe_rule_stat_t;

/* The worker's one-entry neighbour caches, reference include/worker.h:56-63 (worker_t fields
 * last_arp_ip / last_arp_mac / last_ndp_ip / last_ndp_mac).  A calloc'd worker starts all-zero. */
typedef struct {
    uint32_t last_arp_ip;
    uint8_t last_arp_mac[6];
    uint8_t last_ndp_ip[16];
    uint8_t last_ndp_mac[6];
} upe_l1_state_t;

/* Per-worker counters, reference include/worker.h:37-41 plus the control-path tallies the
 * reference does not keep separately.  pkts_forwarded counts FWD verdicts (queued for TX); with
 * the reference's TX stub (tests/benchmark_throughput.c:37-42) that equals its forwarded count. */
typedef struct {
    uint64_t pkts_in;
    uint64_t pkts_parsed;
    uint64_t pkts_matched;
    uint64_t pkts_forwarded;
    uint64_t pkts_dropped;
    uint64_t pkts_consumed; /* NDP NS/NA eaten by handle_control_packet (src/worker.c:96-98) */
    uint64_t arp_learn;     /* ARP packets that reach arp_update (src/worker.c:31-35) */
    uint64_t arp_reply;     /* ARP requests answered in place (src/worker.c:40-52) */
} upe_counters_t;

/* ------------------------------------------------------------------------------------------ */
/* Per-packet verdict word                                                                     */
/* ------------------------------------------------------------------------------------------ */
/* bits 0-3  : verdict code (which exit of process_packet the packet took)
 * bits 4-7  : flags
 * bits 8-31 : index of the matched rule in the caller's sorted rules[] array, plus one
 *             (0 = no rule matched).  rules[idx].rule_id indexes rule_stats. */
enum {
    UPE_V_DROP_PARSE = 0,   /* parse_flow_key failed   src/worker.c:117-125 */
    UPE_V_DROP_NOMATCH = 1, /* no rule                 src/worker.c:130-137 */
    UPE_V_DROP_RULE = 2,    /* ACT_DROP                src/worker.c:146-153 */
    UPE_V_DROP_TTL = 3,     /* TTL / hop limit <= 1    src/worker.c:165-172, 204-211 */
    UPE_V_FWD = 4,          /* queued for TX           src/worker.c:155-244 */
    UPE_V_CONSUMED = 5,     /* NDP NS/NA consumed      src/worker.c:57-100 */
    UPE_V_DROP_ACTION = 6   /* unknown action type     src/worker.c:247-252 */
};
enum {
    UPE_VF_NEIGH_HIT = 0x10, /* MACs rewritten: dst = neighbour MAC, src = port MAC */
    UPE_VF_ARP_LEARN = 0x20, /* well-formed ARP: caller must arp_update(spa, sha) */
    UPE_VF_ARP_REPLY = 0x40, /* ARP request for our IPv4: frame rewritten in place into the
                                reply; caller must tx_send it */
    UPE_VF_L1_INIT = 0x80    /* forwarded v4/v6 packet whose destination equals the L1 cache
                                address the batch started with (ARP: and that address != 0) */
};
#define UPE_VERDICT_CODE(v) ((v) & 0xFu)
#define UPE_VERDICT_RULE(v) ((int64_t)((v) >> 8) - 1)

/* ------------------------------------------------------------------------------------------ */
/* Batch layout in GPU memory                                                                  */
/* ------------------------------------------------------------------------------------------ */
/* frames : one device buffer holding the frames back to back.  Every frame starts on a 16-byte
 *          boundary, and at least UPE_FRAME_TAIL readable bytes must follow each frame start
 *          (pad the buffer end).  Bytes at or beyond a frame's length are never used.
 * desc[i]: (byte_offset << 16) | len, len <= 65535, byte_offset a multiple of 16 below 2^36.
 *          A frame may be a header window shorter than len as long as it holds the first
 *          min(len, UPE_HDR_WINDOW) bytes.
 * verdict: n uint32 words, written by the kernel.
 * A batch is one constant-table segment: control packets (ARP, NDP NS/NA) in it are classified
 * exactly, but their table updates are applied by the caller after the batch (split batches at
 * control packets for exact sequential semantics). */
#define UPE_HDR_WINDOW 96
#define UPE_FRAME_TAIL 96
#define UPE_DESC(off, len) ((((uint64_t)(off)) << 16) | ((uint64_t)(len) & 0xFFFFu))

/* Result summary of the last processed batch. */
typedef struct {
    upe_counters_t counters; /* this batch only */
    uint64_t n_ctrl;         /* control packets (ARP + NDP NS/NA) in the batch */
    uint64_t first_ctrl;     /* index of the first one, or UINT64_MAX */
} upe_batch_info_t;

typedef struct upe_gpu_ctx upe_gpu_ctx_t;

/* ------------------------------------------------------------------------------------------ */
/* Entry points                                                                                */
/* ------------------------------------------------------------------------------------------ */

/* Last error message of the calling thread ("" if none). */
const char *upe_gpu_last_error(void);

/* Number of visible GPUs, or -1. */
int upe_gpu_device_count(void);

/* Host CPUs local to a GPU (its PCI function's NUMA node, sysfs local_cpulist) that the process
 * may run on (its affinity when the library was loaded): up to `cap` of them into cpus (may be
 * NULL), *numa_node (may be NULL) = the node or -1.  Returns how many there are, or -1. */
int upe_gpu_local_cpus(int device, int *cpus, size_t cap, int *numa_node);

/* Pin the calling thread to the slot-th CPU local to `device` (modulo their number), as the
 * reference pins each worker thread (affinity_pin_self, src/affinity.c:48; assign_cores,
 * src/main.c:143-175).  Pinned host buffers allocated afterwards by this thread come from the
 * GPU's NUMA node.  Returns the CPU, or -1. */
int upe_gpu_pin_self(int device, int slot);

/* Open a context on `device`, with its own HIP stream.  Replaces the per-worker state set up by
 * worker_init() (reference src/worker.c:309-330): counters, rule_stats sized by
 * rule_capacity (= rt->capacity, src/worker.c:326), calloc'd L1 caches. */
upe_gpu_ctx_t *upe_gpu_open(int device, size_t rule_capacity);
void upe_gpu_close(upe_gpu_ctx_t *ctx);

/* Upload the rule table: rules[0..count) in the order rule_table_t keeps them (sorted by
 * (priority, rule_id), reference src/rule_table.c:96-109,158).  Replaces the read-only borrow of
 * w->rt (src/worker.c:129).  count <= rule capacity given at open, every rule_id < capacity. */
int upe_gpu_load_rules(upe_gpu_ctx_t *ctx, const upe_rule_t *rules, size_t count);

/* Rule reload with the reference's SIGHUP semantics (src/main.c:216-282: a new table, a fresh
 * calloc'd rule_stats of the new table's capacity per worker, w->rt and w->rule_stats swapped
 * between two bursts; pkts_* and the L1 neighbour caches untouched).  The batches queued so far
 * finish with the old table; if old_stats is given, rule_stats[0..old_capacity) as they stand
 * then (indexed by the OLD table's rule_ids, what the stats thread last printed) are copied out
 * — the reference frees them after its grace period.  The next batch runs with rules[0..count)
 * (sorted, as for upe_gpu_load_rules; rule_id < rule_capacity) and rule_stats all zero, sized
 * rule_capacity (upe_gpu_get_stats reads that many from now on).  Counters and the L1 state
 * carry on.  Arguments are checked before anything changes.  Synchronous; 0 / -1. */
int upe_gpu_reload_rules(upe_gpu_ctx_t *ctx, const upe_rule_t *rules, size_t count,
                         size_t rule_capacity, upe_rule_stat_t *old_stats, size_t old_capacity);

/* The same reload in two halves (round 6), so that the table is built where the reference
 * builds it — in the stats thread, before the swap, while the workers keep forwarding
 * (src/main.c:222-257) — and the worker thread only uploads it between two bursts.
 * upe_rules_compile: the compiled table (rule words, family lists, tuple-space index or decision
 * tree) of `count` sorted rules for a rule_stats of rule_capacity entries; host only (no
 * context, no GPU), any thread; NULL on error (upe_gpu_last_error() on the calling thread).  The
 * build is what dominates a reload of a large table: 0.4 ms (1k rules, scanned) to ~300 ms
 * (16k flow rules, decision tree) on the GPU box's host.
 * upe_gpu_reload_image: upe_gpu_reload_rules() with that image (the capacity is the image's);
 * the image is not consumed.  upe_rules_image_free: NULL is a no-op. */
typedef struct upe_rule_image upe_rule_image_t;
upe_rule_image_t *upe_rules_compile(const upe_rule_t *rules, size_t count, size_t rule_capacity);
int upe_gpu_reload_image(upe_gpu_ctx_t *ctx, const upe_rule_image_t *image,
                         upe_rule_stat_t *old_stats, size_t old_capacity);
void upe_rules_image_free(upe_rule_image_t *image);

/* How the loaded table is classified: 0 = linear first-match scan (tables of up to 64 rules, or
 * a table whose tree outgrew its node budget), 1 = tuple-space index (large tables whose rules
 * fall into few mask signatures: one hash probe per signature, visited in order of each
 * signature's first rule), 2 = decision tree over the per-family rule lists (every other table
 * past 64 rules: a walk to a leaf, then the few rules listed there in order).  Each gives the
 * first match in (priority, rule_id) order (reference src/rule_table.c:163-176).  -1 on error. */
int upe_gpu_rule_index_kind(upe_gpu_ctx_t *ctx);

/* The decision tree of the loaded table (all zero when it has none). */
typedef struct {
    uint64_t nodes;        /* nodes of both families' trees */
    uint64_t leaf_entries; /* rule positions listed in the leaves */
    uint32_t depth4;       /* deepest leaf of the IPv4 tree */
    uint32_t depth6;       /* deepest leaf of the IPv6 tree */
    uint32_t max_leaf;     /* longest leaf list */
    uint32_t trees;        /* trees of the IPv4 forest | trees of the IPv6 forest << 16 */
} upe_rule_index_info_t;
int upe_gpu_rule_index_info(upe_gpu_ctx_t *ctx, upe_rule_index_info_t *info);

/* rule_table_match (reference src/rule_table.c:163-176) over n keys on the host, through the
 * decision tree the GPU path builds for rules[0..count) (sorted as for upe_gpu_load_rules; the
 * walk is the device's, bit for bit), or the per-family linear first match when the table gets
 * no tree.  out[i] = the sorted index of keys[i]'s first matching rule, or -1 (no match, or an
 * ip_ver other than 4 / 6).  info (optional): the tree's shape.  No GPU needed.  0 / -1. */
int upe_rules_match_host(const upe_rule_t *rules, size_t count, const upe_flow_key_t *keys,
                         size_t n, int64_t *out, upe_rule_index_info_t *info);

/* upe_gpu_resolve_keys' host twin (upe_host.c): arp_get_mac / ndp_get_mac over n keys, the
 * reference's linear probe restated over the caller's slot arrays themselves (power-of-two
 * capacities, or NULL with capacity 0: every lookup of that family misses) — no index is built.
 * mac[i] in upe_gpu_resolve_keys' format.  No GPU needed.  0 / -1 (upe_host_last_error()). */
int upe_neigh_lookup_host(const upe_arp_entry_t *arp, size_t arp_capacity,
                          const upe_ndp_entry_t *ndp, size_t ndp_capacity,
                          const upe_flow_key_t *keys, size_t n, uint64_t *mac);

/* Flow keys on the device, apart from the classify launch (csrc/upe_keys.hip): the two reference
 * entry points callers use on their own.  Both are read-only with respect to the context: the
 * loaded table, rule_stats, the counters, the L1 state and upe_gpu_launch_info are untouched, and
 * no launch is counted.  n == 0 is a successful no-op; a null context, a null buffer with n > 0
 * or an n above 2^32 - 257 fails (-1, upe_gpu_last_error()) before anything is launched.
 *
 * parse_flow_key (src/parser.c:6-111; the RX thread's call, src/rx_pcap.c:71-72) over a resident
 * batch ("Batch layout", the UPE_FRAME_TAIL rule of upe_gpu_process).  Frames are read only.
 * Plain parse_flow_key, not the worker's control-packet handling: an ARP frame and an ICMPv6
 * NS/NA both fail to parse (ethertype 0x0806; protocol 58).  Success: d_rc[i] = 0 and d_keys[i] =
 * the 44 bytes the parser leaves in a key zeroed beforehand (an IPv4 key's union bytes 4-15 and
 * the padding bytes 1-3 and 41-43 zero; addresses and ports in the reference's byte orders: IPv4
 * host order in .v4, IPv6 wire bytes, ports host order).  Failure: d_rc[i] = -1 and 44 zero bytes,
 * so ip_ver == 0 marks a failed parse when d_rc is NULL.  A byte at or past len never influences
 * a key or a result.  Every byte of d_keys[0..n) is written.  Asynchronous on `stream` (NULL:
 * the context's). */
int upe_gpu_parse_keys(upe_gpu_ctx_t *ctx, const uint8_t *d_frames, const uint64_t *d_desc,
                       size_t n, upe_flow_key_t *d_keys, int32_t *d_rc /* optional */,
                       void *stream);

/* rule_table_match (src/rule_table.c:163-176) over n keys on the device: d_rule[i] = the index,
 * in the sorted rules[] the table was loaded or compiled from, of the first rule that matches
 * d_keys[i], or -1: no rule matches, or ip_ver is neither 4 nor 6 (upe_rules_match_host's
 * convention; the reference's match_rule, src/rule_table.c:76-91, would skip the address test
 * for such a key, and parse_flow_key never produces one).  Of an IPv4 key's addresses only union
 * bytes 0-3 are read; padding never is.  Whichever index the table's compiler chose (or was told
 * to choose: UPE_GPU_TSS, UPE_GPU_TREE, UPE_GPU_TREE_BINTH) is the one that is probed.
 * image == NULL: the context's loaded table; fails when the context holds no rules (none loaded
 * since upe_gpu_open, or an empty table).  Asynchronous on `stream`.
 * With an image (upe_rules_compile), a dry run before upe_gpu_reload_image: the image is uploaded
 * beside the loaded table for the duration of the call, as a reload uploads it but without the
 * swap, and is not consumed (it may be used again, and reloaded).  This form is synchronous: it
 * returns once d_rule is written, and the device copy is gone by then. */
int upe_gpu_match_keys(upe_gpu_ctx_t *ctx, const upe_rule_image_t *image /* NULL: loaded table */,
                       const upe_flow_key_t *d_keys, size_t n, int32_t *d_rule, void *stream);

/* Upload a snapshot of the neighbour tables' slot arrays (arpt->entries / ndpt->entries with
 * their power-of-two capacities).  Lookups probe exactly as arp_get_mac/ndp_get_mac do.
 * Either table may be NULL with capacity 0 (every lookup misses).  All or nothing: the new
 * snapshot is built and uploaded beside the previous one and swapped in once it is whole, so a
 * call that fails (-1: an allocation, a copy, the index placement) keeps the previous snapshot
 * and the context goes on classifying with it.  The price is a peak of old plus new index on the
 * device during the call, 16 bytes per ARP index slot and 32 per NDP index slot. */
int upe_gpu_load_neigh(upe_gpu_ctx_t *ctx, const upe_arp_entry_t *arp, size_t arp_capacity,
                       const upe_ndp_entry_t *ndp, size_t ndp_capacity);

/* The same load in two halves, as the rule reload has them: the snapshot's index is built where
 * the tables change — the thread that runs arp_expire / ndp_expire — and the worker thread only
 * uploads it between two bursts.
 * upe_neigh_compile: the snapshot of the two slot arrays (upe_gpu_load_neigh's arguments, checked
 * the same way: power-of-two capacities, a table wherever there is a capacity); host only (no
 * context, no GPU), any thread; NULL on error (upe_gpu_last_error() on the calling thread) — a bad
 * argument, or the index placement: at most three reachable IPv6 addresses may share one key of
 * the index (fold_v6).  Equal tables give equal images.
 * upe_gpu_load_neigh_image: upe_gpu_load_neigh() with that image — uploaded beside the previous
 * snapshot and swapped in once it is whole; a call that fails (-1) keeps the previous snapshot.
 * The image is not consumed.  upe_neigh_image_free: NULL is a no-op. */
typedef struct upe_neigh_image upe_neigh_image_t;
upe_neigh_image_t *upe_neigh_compile(const upe_arp_entry_t *arp, size_t arp_capacity,
                                     const upe_ndp_entry_t *ndp, size_t ndp_capacity);
int upe_gpu_load_neigh_image(upe_gpu_ctx_t *ctx, const upe_neigh_image_t *image);
void upe_neigh_image_free(upe_neigh_image_t *image);

/* arp_get_mac (src/arp_table.c:55-80) / ndp_get_mac (src/ndp_table.c:67-86) over n keys on the
 * device (csrc/upe_neigh.hip): the next hop of d_keys[i].dst_ip by d_keys[i].ip_ver — 4: the ARP
 * table, asked for union bytes 0-3 as a little-endian word (dst_ip.v4; bytes 4-15 are never read);
 * 6: the NDP table, asked for the 16 bytes; anything else: not found.  d_mac[i] = the MAC's six
 * bytes in bits 0-47 (byte 0 lowest: a memcpy of the MAC into a zeroed little-endian uint64_t)
 * with bit 48 set, or exactly 0 when the address is not found.  Answers are those of the
 * reference's probe over the slot arrays the snapshot was built from: an entry no probe reaches
 * is not found, of one address in two slots the one the probe meets first answers, a stale
 * address in an invalid slot is not found.  The table function alone: no L1 cache (the zero guard
 * of src/worker.c:186 is the worker's; 0.0.0.0 and :: are ordinary addresses here), no TTL check,
 * no rule; the counters, rule_stats, the L1 state and upe_gpu_launch_info are untouched and no
 * launch is counted.
 * image == NULL: the context's loaded snapshot.  Asynchronous on `stream` (NULL: the context's),
 * one launch; the caller lets it finish (upe_gpu_sync) before the next upe_gpu_load_neigh or
 * upe_gpu_load_neigh_image when the stream is one of its own.
 * With an image (upe_neigh_compile), a dry run before upe_gpu_load_neigh_image: the image is
 * uploaded beside the loaded snapshot for the duration of the call, without the swap, and is not
 * consumed.  This form is synchronous: it returns once d_mac is written, and the device copy is
 * gone by then.
 * n == 0 launches nothing.  -1 (upe_gpu_last_error()) before any launch: a NULL context; NULL
 * d_keys or d_mac with n > 0; d_keys not 4-byte or d_mac not 8-byte aligned; n above 2^32 - 257. */
int upe_gpu_resolve_keys(upe_gpu_ctx_t *ctx,
                         const upe_neigh_image_t *image /* NULL: the loaded snapshot */,
                         const upe_flow_key_t *d_keys, size_t n, uint64_t *d_mac, void *stream);
#define UPE_MAC_FOUND (1ull << 48) /* set in d_mac[i] / mac[i] on a hit */

/* The TX port identity the worker reads from tx_ctx_t (include/tx.h:9-14): own MAC (source MAC of
 * forwarded frames, src/worker.c:199,229) and own IPv4 (ARP replies, src/worker.c:40). */
int upe_gpu_set_port(upe_gpu_ctx_t *ctx, const uint8_t eth_addr[6], uint32_t ip4_addr);

/* L1 neighbour-cache state (kept on the device between batches). */
int upe_gpu_set_l1(upe_gpu_ctx_t *ctx, const upe_l1_state_t *l1);
int upe_gpu_get_l1(upe_gpu_ctx_t *ctx, upe_l1_state_t *l1);

/* Process one batch resident in GPU memory (see "Batch layout").  Asynchronous on `stream`
 * (a hipStream_t; NULL = the context's own stream).  Frames are rewritten in place exactly as
 * process_packet rewrites b->data.  Counters, rule stats and the L1 state accumulate in the
 * context, as they do in worker_t. */
int upe_gpu_process(upe_gpu_ctx_t *ctx, uint8_t *d_frames, const uint64_t *d_desc,
                    uint32_t *d_verdict, size_t n, void *stream);

/* Rewritten-header record (emit mode), 16 bytes per packet.  process_packet rewrites at most
 * three places of a forwarded frame (src/worker.c:162-244): bytes 0..11 (dst MAC = the next-hop
 * MAC and src MAC = tx->eth_addr on a neighbour hit), the TTL (IPv4 byte 22) with the header
 * checksum (bytes 24..25), or the hop limit (IPv6 byte 21).  Emit mode leaves the frame alone
 * and writes those bytes here instead, one coalesced 16-byte store per packet:
 *   b[0..11]  bytes 0..11 of the forwarded frame (the original MACs when the lookup missed)
 *   b[12]     new TTL (IPv4) or hop limit (IPv6)
 *   b[13..14] new IPv4 header checksum as stored at frame bytes 24..25 (0 for IPv6)
 *   b[15]     4 or 6: the packet was forwarded (verdict code UPE_V_FWD) as that family
 * upe_hdr_apply(frame, rec) turns a frame into exactly the bytes process_packet leaves in
 * b->data; it does nothing when b[15] == 0.
 *
 * Layout of a launch's records (round 5): only forwarded packets get one, compacted per 64-packet
 * group in packet order — forwarded packet i's record is rec[64 * (i / 64) + k], k = the number
 * of forwarded packets before it among packets 64 * (i / 64) .. i - 1 (the kernel's ballot and
 * lane count; a reader walking the verdicts in order keeps a cursor, reset to i at every multiple
 * of 64).  The other slots are not written.  UPE_HDR_SLOT gives the slot from that count.
 *
 * BREAKING CHANGE in layout 2 (round 5): layout 1 (rounds 1-4) wrote one record per packet at
 * rec[i], zero for packets not forwarded.  A caller that reads rec[i] per packet applies wrong or
 * stale records under layout 2 without any error: it must walk with the cursor above (or
 * UPE_HDR_SLOT), or check UPE_HDR_LAYOUT at compile time and upe_gpu_hdr_layout() at run time
 * (the library it actually loaded) before trusting either form. */
#define UPE_HDR_LAYOUT 2
#define UPE_HDR_SLOT(i, k) ((((size_t)(i)) & ~(size_t)63) + (size_t)(k))
int upe_gpu_hdr_layout(void);   /* UPE_HDR_LAYOUT of the loaded library */
typedef struct {
    uint8_t b[16];
} upe_hdr_rec_t;

/* upe_gpu_process() in emit mode: d_hdr (device, room for n records, 16-byte aligned) receives
 * the forwarded packets' rewritten header bytes (the record layout above) and the frames are not
 * written — except the ARP requests answered
 * in place (UPE_VF_ARP_REPLY), which the reference transmits at once (src/worker.c:40-52).
 * Verdicts, counters, rule_stats and the L1 state are exactly those of upe_gpu_process().  This
 * is the layout for a TX path that sends header and payload as separate pieces (sendmmsg
 * iovecs, or a NIC gather list) and for host round trips, which then copy back 16 bytes per
 * packet instead of the header span; in-place rewriting of 64-byte frames costs the path the
 * partial 128-byte lines it dirties. */
int upe_gpu_process_emit(upe_gpu_ctx_t *ctx, uint8_t *d_frames, const uint64_t *d_desc,
                         uint32_t *d_verdict, upe_hdr_rec_t *d_hdr, size_t n, void *stream);

/* A ring of `count` resident batches of n packets each in ONE launch (throughput mode): the
 * batches lie back to back in the "Batch layout" (batch j = descriptors, verdicts and records
 * [j*n, (j+1)*n), frames anywhere in d_frames) and are classified in ring order by one
 * persistent launch in emit mode, so the per-launch cost (dispatch, the first windows' round
 * trip, the tail, the boundary) is paid once per ring, not once per batch.  Counters,
 * rule_stats, the L1 state, every verdict code and every record equal those of `count`
 * back-to-back upe_gpu_process_emit() calls over the batches (record slots are counted from the
 * ring's first packet; n is a multiple of 64, so each batch's records stay in its own range);
 * UPE_VF_L1_INIT is relative to the ring's start.  n a multiple of 1024, n * count <= 2^24 (on a device or
 * partition of fewer than 256 CUs, with a table of up to 4092 rules: <= 65536 * CUs, the most one
 * launch takes there).  d_done_ns (optional, device or
 * host-mapped, count entries): for each batch, the time (ns) from the launch's first workgroup
 * to the moment its last workgroup had issued the batch's last stores — per-batch completion
 * latency — or 0 where not stamped (stamps need a linear-scan table, batches of at least
 * one tile per persistent workgroup, 256k packets on MI355X, and at most 64 batches per
 * workgroup's share).  A stamp excludes the launch's final repair of look-back candidates that
 * waves deferred (launch_info().deferred > 0, only when another kernel holds CUs): such a
 * batch's last verdicts and records are final when the launch completes, not at its stamp.
 * Asynchronous on `stream`. */
int upe_gpu_process_ring_emit(upe_gpu_ctx_t *ctx, uint8_t *d_frames, const uint64_t *d_desc,
                              uint32_t *d_verdict, upe_hdr_rec_t *d_hdr, size_t n, size_t count,
                              uint64_t *d_done_ns, void *stream);

/* Apply one record to its frame (host; src/worker.c:174-176,197-200,213,227-230 as bytes). */
void upe_hdr_apply(uint8_t *frame, const upe_hdr_rec_t *rec);

/* Host round trip: process n packets that live in HOST memory, the way the path runs between
 * libpcap (reference src/rx_pcap.c:42-93 fills pktbufs in host memory) and AF_PACKET TX
 * (src/tx_afpacket.c:78-118 sends from host memory).  The batch is cut into chunks of `chunk`
 * packets (0 = 256k) pipelined through a ring of device slots (4; UPE_GPU_HOST_SLOTS): chunk k+1's frames and descriptors go
 * host->device on a copy stream while chunk k is classified on the context's stream and chunk
 * k-1's verdicts and rewritten header bytes go device->host on a second copy stream.  Chunks are
 * classified in order, so counters, rule_stats and the L1 state evolve exactly as for
 * back-to-back upe_gpu_process() batches of `chunk` packets (upe_gpu_batch_info() describes the
 * last chunk).  h_frames / h_desc follow the "Batch layout" (offsets relative to h_frames,
 * frames_bytes covering UPE_FRAME_TAIL bytes past every frame start); a frame may be a header
 * window (UPE_HDR_WINDOW), which is how a caller avoids shipping payloads.  Only the first
 * min(len, UPE_REWRITE_EXTENT) bytes of a frame can change; those are copied back in place.
 * Synchronous.  Buffers from upe_gpu_host_alloc() (pinned) give the full PCIe rate; pageable
 * buffers work at the staged-copy rate. */
#define UPE_REWRITE_EXTENT 48
int upe_gpu_process_host(upe_gpu_ctx_t *ctx, uint8_t *h_frames, size_t frames_bytes,
                         const uint64_t *h_desc, uint32_t *h_verdict, size_t n, size_t chunk);

/* The host round trip in emit mode (chunk 0 = 128k packets): the same pipeline, but only the verdicts and the 16-byte
 * rewritten-header records come back (h_hdr, room for n records in the layout above, counted
 * from the batch's first packet; chunks are whole 64-packet groups; each chunk's records come back
 * in one copy of the device array, so every slot of h_hdr[0 .. n) is written, and a slot that holds
 * no record — "not written" by the kernel in the layout above — comes back with unspecified bytes:
 * read h_hdr through the verdicts, as for any launch; pinned for the full rate: 20 bytes per
 * packet over the link instead of the frames' rewritten span — the link's two directions share
 * its bandwidth, so fewer bytes back let the frames go in faster).  apply_threads >= 0: the
 * records are applied to h_frames on the host (upe_hdr_apply, answered ARP requests copied back)
 * by the calling thread plus `apply_threads` pool threads pinned near the GPU, two chunks behind
 * the copies, so that on return h_frames, h_verdict, counters, rule_stats and the L1 state are
 * exactly those of upe_gpu_process_host(); apply_threads = -1 leaves the frames as they were
 * except the answered ARP requests (as upe_gpu_process_emit does; a TX path that sends each
 * record as its own iovec).  Synchronous.  0 / -1. */
int upe_gpu_process_host_emit(upe_gpu_ctx_t *ctx, uint8_t *h_frames, size_t frames_bytes,
                              const uint64_t *h_desc, uint32_t *h_verdict, upe_hdr_rec_t *h_hdr,
                              size_t n, size_t chunk, int apply_threads);

/* Egress (reference src/worker.c:240-243, 287-303 and src/tx_afpacket.c:78-118): the forwarded
 * frames of a classified host batch (verdict code UPE_V_FWD, frames as the path left them —
 * rewritten in place, or with the emit records applied by upe_hdr_apply), in packet order, handed
 * to `send` the way the reference's worker loop flushes them: one call per input burst of `burst`
 * packets that forwarded anything (WORKER_BURST_SIZE = 32 in the reference; at most
 * UPE_TX_BATCH_MAX = 64 frames per call, the sendmmsg cap of src/tx_afpacket.c:82-84).  `send` has
 * tx_send_batch's contract with a user pointer first: it returns the frames it sent (negative
 * counts as 0).  *forwarded += sent and *dropped += count - sent, as the worker counts them
 * (src/worker.c:290-294); the caller then frees every buffer of the batch.  0, or -1 for a bad
 * argument (burst 0 or above UPE_TX_BATCH_MAX). */
#define UPE_TX_BATCH_MAX 64
typedef int (*upe_tx_batch_fn)(void *user, const uint8_t *const *frames, const size_t *lens,
                               int count);
int upe_tx_flush(const uint8_t *h_frames, const uint64_t *h_desc, const uint32_t *h_verdict,
                 size_t n, size_t burst, upe_tx_batch_fn send, void *user, uint64_t *forwarded,
                 uint64_t *dropped);
/* The same TX calls from the grouped egress list of upe_gpu_process_emit_tx (h_tx, h_tx_count
 * copied to the host) instead of the verdicts: no per-packet verdict scan; the same calls,
 * arguments and accounting as upe_tx_flush. */
int upe_tx_flush_groups(const uint8_t *h_frames, const uint64_t *h_desc, const uint32_t *h_tx,
                        const uint32_t *h_tx_count, size_t n, size_t burst, upe_tx_batch_fn send,
                        void *user, uint64_t *forwarded, uint64_t *dropped);

/* ------------------------------------------------------------------------------------------ */
/* The GPU-backed worker loop (upe_amd/csrc/upe_worker.c, C)                                   */
/* ------------------------------------------------------------------------------------------ */
/* What the loop needs from the program around it: the callees of reference worker_main /
 * process_packet (SURVEY.md §8(b) "Callees"), as callbacks with a user pointer first.  A packet
 * buffer is an opaque handle (a pktbuf_t *). */
typedef struct upe_worker_ops {
    /* ring_pop_burst (src/ring.c:53): up to `max` handles into bufs, returns how many */
    unsigned (*pop_burst)(void *user, void **bufs, unsigned max);
    /* g_stop (src/worker.c:18), read only when the ring is empty, as src/worker.c:270-273 */
    int (*stop)(void *user);
    /* a handle's frame: b->data and b->len (include/pktbuf.h:10-14) */
    uint8_t *(*data)(void *user, void *buf);
    size_t (*len)(void *user, void *buf);
    /* pktbuf_free (src/pktbuf.c:324) */
    void (*free_buf)(void *user, void *buf);
    /* tx_send / tx_send_batch (src/tx_afpacket.c:60-118) */
    int (*tx_send)(void *user, const uint8_t *frame, size_t len);
    int (*tx_send_batch)(void *user, const uint8_t *const *frames, const size_t *lens, int count);
    /* handle_control_packet's table writes (src/worker.c:30-39, 64-95): arp_update(ip host
     * order, mac), ndp_update(ip, mac); then the loop calls load_neigh so that the next packet
     * sees the write: the callee uploads the tables (upe_gpu_load_neigh under its locks) */
    void (*arp_update)(void *user, uint32_t ip, const uint8_t mac[6]);
    void (*ndp_update)(void *user, const uint8_t ip[16], const uint8_t mac[6]);
    int (*load_neigh)(void *user, upe_gpu_ctx_t *ctx);
    /* optional: polled after every pop; nonzero = the program changed something the context
     * holds (a SIGHUP rule swap, src/main.c:258-265; neighbour expiry, src/main.c:205-214): the
     * loop finishes the packets popped before with the old state, then calls sync(), which
     * makes the change (upe_gpu_reload_rules, upe_gpu_load_neigh), and classifies the burst just
     * popped with the new state.  A nonzero return of sync() ends the loop with -1. */
    int (*poll)(void *user);
    int (*sync)(void *user, upe_gpu_ctx_t *ctx);
    /* optional: after every GPU batch walked, and after every sync(), the loop's counters so far
     * (the worker_t fields the stats thread reads, src/main.c:284-315: pkts_in, pkts_parsed,
     * pkts_matched, pkts_forwarded, pkts_dropped; the rest as upe_counters_t defines them).
     * ctx is NULL while a later batch is still on the GPU: the context's statistics then already
     * hold some packets the counters do not, so publish the counters only (and never call into
     * the context, which would wait for that batch).  ctx is the context when nothing is in
     * flight — after a drain (empty ring, a table-writing packet, a polled change) and at least
     * every 32 batches of a stream that never drains — and upe_gpu_get_stats(ctx, ...) then
     * matches the counters packet for packet (rule_stats packets sum to pkts_matched). */
    void (*publish)(void *user, upe_gpu_ctx_t *ctx, const upe_counters_t *counters);
    /* optional: the handles of a burst's forwarded frames after its tx_send_batch, in one call
     * (else free_buf on each; src/worker.c:300-302 frees them one by one) */
    void (*free_burst)(void *user, void *const *bufs, unsigned count);
} upe_worker_ops_t;

typedef struct {
    size_t batch;       /* most packets per GPU batch (0 = 65536) */
    unsigned burst;     /* most handles per pop (0 = 32, WORKER_BURST_SIZE; at most 64) */
    /* NULL: each packet's first UPE_HDR_WINDOW bytes are copied into pinned staging and
     * classified there by upe_gpu_process_mapped_emit (the kernel reads the windows over the
     * link; no DMA copies), the verdicts and records written to pinned host memory (records
     * applied to the buffers in the walk).  Non-NULL: every buffer's frame lies at
     * pool_base + a multiple of 16, inside memory registered with upe_gpu_host_register (e.g.
     * the reference's pktbuf pool), and each batch is classified where it lies by
     * upe_gpu_process_mapped_emit (nothing copied; the records, written to pinned host memory,
     * applied to the buffers in the walk). */
    uint8_t *pool_base;
    unsigned idle_ns;   /* sleep when the ring is empty and nothing is held (0 = 1000, as
                           src/worker.c:274-277) */
    size_t pool_bytes;  /* with pool_base: the registered region's size; a frame whose bytes
                           (at least UPE_FRAME_TAIL of them, what the kernel may read) do not lie
                           inside it stops the loop with an error instead of reaching the GPU */
} upe_worker_cfg_t;

/* The GPU-backed replacement of worker_main (reference src/worker.c:255-307), on the calling
 * thread, until the ring is empty with ops->stop() set.  Pops bursts and gathers them into GPU
 * batches, classified by the context's tables; a batch is cut after every packet that writes a
 * neighbour table (ARP, NS/NA), whose write is applied through ops before the next packet is
 * classified, and also run at once whenever the ring is empty.  Then, per popped burst and in
 * packet order, exactly the calls worker_main makes: tx_send of each answered ARP request,
 * free_buf of each dropped or consumed packet (pkts_dropped += 1 for a drop), and one
 * tx_send_batch of the burst's forwarded frames (rewritten as process_packet leaves them) with
 * pkts_forwarded += sent, pkts_dropped += count - sent, and free_buf of each.  *counters
 * (optional) receives the loop's counters at the end (they start from zero).  0, or -1 on a
 * GPU, callback or argument error (upe_gpu_last_error()). */
int upe_gpu_worker_run(upe_gpu_ctx_t *ctx, const upe_worker_ops_t *ops, void *user,
                       const upe_worker_cfg_t *cfg, upe_counters_t *counters);

/* Pinned (page-locked) host memory for upe_gpu_process_host() batches; the GPU can also read and
 * write it directly (upe_gpu_process_mapped). */
void *upe_gpu_host_alloc(size_t bytes);
int upe_gpu_host_free(void *ptr);

/* Page-lock an existing host buffer and map it for the GPU (e.g. the reference's pktbuf pool,
 * src/pktbuf.c: pool->mem), so that upe_gpu_process_mapped() can classify its frames where they
 * lie.  `ptr` and `bytes` need no alignment.  0 / -1. */
int upe_gpu_host_register(void *ptr, size_t bytes);
int upe_gpu_host_unregister(void *ptr);

/* The batch in host memory, classified by the kernel's own loads over the link: no DMA copies and
 * no staging slots.  The kernel reads each frame's header window and its descriptor from host
 * memory and writes the verdicts (and in place: the rewritten header bytes, exactly as
 * upe_gpu_process() does in HBM; emit: the 16-byte records) straight into host memory, so only
 * the bytes the path touches cross the link — for long frames a fraction of the frame span the
 * DMA round trip must copy.  Every pointer is host memory from upe_gpu_host_alloc() or
 * upe_gpu_host_register() (checked: -1 otherwise); layout and UPE_FRAME_TAIL rule as for
 * upe_gpu_process().  Asynchronous on `stream` like upe_gpu_process(): the outputs are the
 * host's to read after upe_gpu_sync().  This replaces the worker's burst loop over pktbufs in the
 * pool (src/worker.c:255-307) with nothing copied: the frames are rewritten where tx_send reads
 * them (src/tx_afpacket.c:60-76). */
int upe_gpu_process_mapped(upe_gpu_ctx_t *ctx, uint8_t *h_frames, const uint64_t *h_desc,
                           uint32_t *h_verdict, size_t n, void *stream);
int upe_gpu_process_mapped_emit(upe_gpu_ctx_t *ctx, uint8_t *h_frames, const uint64_t *h_desc,
                                uint32_t *h_verdict, upe_hdr_rec_t *h_hdr, size_t n,
                                void *stream);

/* Queue `count` batches back to back from native code: batch k is d_frames_list[k] (a host
 * array of device pointers), all sharing one descriptor array and one verdict array (each batch
 * overwrites the verdicts of the one before).  Equivalent to `count` upe_gpu_process() calls,
 * without a caller round trip per batch; what a GPU-backed worker thread does with a ring of
 * resident batch buffers. */
int upe_gpu_process_batches(upe_gpu_ctx_t *ctx, uint8_t *const *d_frames_list,
                            const uint64_t *d_desc, uint32_t *d_verdict, size_t n, size_t count,
                            void *stream);
/* The same in emit mode (every batch writes its records to d_hdr): upe_gpu_process_queue_emit()
 * over `count` batches that share d_desc, d_verdict and d_hdr. */
int upe_gpu_process_batches_emit(upe_gpu_ctx_t *ctx, uint8_t *const *d_frames_list,
                                 const uint64_t *d_desc, uint32_t *d_verdict,
                                 upe_hdr_rec_t *d_hdr, size_t n, size_t count, void *stream);

/* One resident batch of a queue: device frames, descriptors, verdicts and records, n packets. */
typedef struct upe_gpu_batch {
    uint8_t *frames;
    const uint64_t *desc;
    uint32_t *verdict;
    upe_hdr_rec_t *hdr;
    size_t n;
} upe_gpu_batch_t;

/* The worker loop (reference src/worker.c:255-307: burst after burst, the worker's state carried
 * from one to the next) over `count` resident batches in emit mode, one launch per batch queued
 * from native code on `stream`.  Results — every verdict, record, counter, rule_stats word and
 * the L1 state — equal `count` upe_gpu_process_emit() calls in order; batches may differ in size
 * (an empty one is a no-op) and may share descriptor and output buffers.  Every batch is
 * checked (a batch of n > 0 packets needs its records) before any is queued.  0 / -1. */
int upe_gpu_process_queue_emit(upe_gpu_ctx_t *ctx, const upe_gpu_batch_t *batches, size_t count,
                               void *stream);

/* upe_gpu_process() plus software RSS in the same pass (reference src/rx_pcap.c:67-77 parses
 * every packet a second time on the RX thread for this): d_flow_hash[i] (device, n uint32) =
 * flow_hash() of the packet's flow key (src/parser.c:113-135) when parse_flow_key succeeds, 0
 * otherwise (verdict code DROP_PARSE or CONSUMED says which; a parsed packet can hash to 0 too).
 * The hash alone does not give the worker ring: the RX thread sends a packet that parses to ring
 * hash & (rings - 1) and every other packet to the ring its round-robin cursor names
 * (src/rx_pcap.c:19-25,74-77).  upe_gpu_rx_dispatch below makes that choice, and it runs before
 * any worker has classified (and rewritten) the frames. */
int upe_gpu_process_rss(upe_gpu_ctx_t *ctx, uint8_t *d_frames, const uint64_t *d_desc,
                        uint32_t *d_verdict, uint32_t *d_flow_hash, size_t n, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Ingress batch: a burst of pktbuf handles gathered on the device                             */
/* ------------------------------------------------------------------------------------------ */
/* The first stage: from what the reference hands a worker — a burst of pktbuf_t * handles into a
 * pool of fixed-size buffers (include/pktbuf.h:8-14, src/worker.c:255-307) — to the "Batch
 * layout" every other call here starts from, without the host touching a frame byte.  A handle
 * is passed as its buffer index (b - pool->buffers).
 *
 * The pool.  Buffer s is the `stride` bytes at pool + s * stride: a 64-bit timestamp at 0, a
 * 64-bit len at 8 and stride - 16 data bytes from 16 (pktbuf_t with stride = sizeof(pktbuf_t) =
 * 2064; other strides serve small pools).  stride is a multiple of 16 and at least
 * 16 + UPE_FRAME_TAIL; pool_bytes is at least stride and at most 2^36; pool is 16-byte aligned,
 * in device memory or in host memory from upe_gpu_host_alloc / upe_gpu_host_register.  The
 * kernels only load from it.  A slot may appear more than once, and slots need not ascend.
 *
 * A handle is bad when (uint64_t)s * stride + stride > pool_bytes (its buffer is then not
 * read), or its len > stride - 16, or its len > 65535; len is compared as 64 bits.  A bad handle
 * keeps its position k: it gets a descriptor of len 0 (offset k * UPE_HDR_WINDOW in WINDOW mode,
 * 16 in REF and FULL mode), takes 0 bytes of d_out in FULL mode and an all-zero window in WINDOW
 * mode, is never a control packet, and is counted in `bad`; its timestamp is the buffer's, or 0
 * when the slot lies outside the pool.  The caller looks at info.bad before classifying.
 *
 * Modes.
 *   UPE_INGRESS_REF     nothing is copied: d_desc[k] = UPE_DESC(s_k * stride + 16, len_k),
 *                       relative to pool; the caller classifies the frames where they lie.
 *                       bytes = need = 0.
 *   UPE_INGRESS_WINDOW  d_out + k * UPE_HDR_WINDOW receives the frame's first
 *                       min(len_k, UPE_HDR_WINDOW) bytes, then zeros to the window's end;
 *                       d_desc[k] = UPE_DESC(k * UPE_HDR_WINDOW, len_k) — the staging layout of
 *                       upe_gpu_worker_run.  Needs out_bytes >= n * UPE_HDR_WINDOW;
 *                       bytes = need = n * UPE_HDR_WINDOW.
 *   UPE_INGRESS_FULL    the packing rule of upe_gpu_egress_pack: frame k starts at o_k = the sum
 *                       over j < k of (len_j + 15) & ~15, d_desc[k] = UPE_DESC(o_k, len_k) (a bad
 *                       handle: UPE_DESC(16, 0)), the frame's bytes are followed by zeros up to
 *                       the next 16-byte boundary.  Frame k is written only if
 *                       o_k + ((len_k + 15) & ~15) <= out_bytes; offsets ascend, so the written
 *                       frames are a prefix, counted in `packed`, and `need` is the size to retry
 *                       with.  d_desc and d_timestamp entries from `packed` on, d_ctrl entries
 *                       naming a position from `packed` on, and anything at or beyond
 *                       d_out + out_bytes are not written.  The UPE_FRAME_TAIL bytes after the
 *                       last frame are the caller's to provide, as for upe_gpu_egress_pack.  The
 *                       only mode whose output upe_gpu_process_segmented and upe_gpu_egress_pack
 *                       accept.
 * In REF and WINDOW mode packed = n.
 *
 * Side outputs.  d_timestamp[k] (optional) = buffer s_k's timestamp, not interpreted.
 * d_ctrl[0 .. n_ctrl) (optional) = the positions k, ascending, of the packets for which
 * handle_control_packet may write a neighbour table (reference src/worker.c:23-104; the rule of
 * upe_gpu_process_segmented's marking pass and of upe_gpu_worker_run): ethertype 0x0806 with
 * bytes 14..19 equal to 00 01 08 00 06 04, or ethertype 0x86DD with len >= 78, byte 20 equal to
 * 58 and byte 54 135 or 136; bytes at or past len read as zero.  Those are where a caller cuts
 * the batch.  bad, first_bad, n_ctrl and first_ctrl count all n handles in every mode, whether or
 * not d_ctrl is given.
 *
 * Frames are read in whole 16-byte quads (the quad holding a frame's last byte is read whole,
 * never a quad past it).  Asynchronous on `stream` (at most three launches; scratch lives in the
 * context, so a context's gathers are queued one after another).  n == 0 zeroes *d_info with
 * first_bad = first_ctrl = UINT64_MAX and launches nothing.  -1 before any launch: a NULL
 * context; a NULL required pointer with n > 0 (d_info always); an unknown mode; stride or
 * pool_bytes outside the rules above, or a pool that is not 16-byte aligned; d_out not 16-byte
 * aligned, given in REF mode or missing in the other modes; out_bytes below n * UPE_HDR_WINDOW
 * in WINDOW mode; n beyond the kernels' 32-bit indexes; a pool that is neither device memory nor
 * pinned, mapped host memory; d_out overlapping the pool in address — a pool in device memory
 * counts up to the end of the allocation that holds it, as d_frames does for
 * upe_gpu_egress_pack.
 * UPE_INGRESS_BLOCK: packets per workgroup of the gather kernels (batch sizes around it are
 * where tests look). */

/* Mirrors pktbuf_t, reference include/pktbuf.h:8-14 (2064 bytes). */
#define UPE_PKTBUF_DATA 2048
typedef struct {
    uint64_t timestamp;
    uint64_t len;
    uint8_t data[UPE_PKTBUF_DATA];
} upe_pktbuf_t;

#define UPE_INGRESS_BLOCK 1024
enum { UPE_INGRESS_REF = 0, UPE_INGRESS_WINDOW = 1, UPE_INGRESS_FULL = 2 };

typedef struct {
    uint64_t packets;    /* n */
    uint64_t packed;     /* FULL: frames written (a prefix in handle order); else n */
    uint64_t bytes;      /* bytes of d_out defined by the call (REF: 0) */
    uint64_t need;       /* bytes all n would use (== bytes when everything fitted) */
    uint64_t bad;        /* handles refused */
    uint64_t first_bad;  /* position k of the first, or UINT64_MAX */
    uint64_t n_ctrl;     /* packets that may write a neighbour table */
    uint64_t first_ctrl; /* position of the first, or UINT64_MAX */
} upe_ingress_info_t;

int upe_gpu_ingress_gather(upe_gpu_ctx_t *ctx, const uint8_t *pool, size_t pool_bytes,
                           size_t stride,
                           const uint32_t *d_slot, size_t n, /* buffer indexes, arrival order */
                           int mode,
                           uint8_t *d_out, size_t out_bytes, /* NULL / 0 in REF mode */
                           uint64_t *d_desc,                 /* n */
                           uint64_t *d_timestamp,            /* n, optional */
                           uint32_t *d_ctrl,                 /* n, optional */
                           upe_ingress_info_t *d_info,       /* device, 64 bytes */
                           void *stream);

/* ------------------------------------------------------------------------------------------ */
/* RX dispatch: spreading a batch over the worker rings                                        */
/* ------------------------------------------------------------------------------------------ */
/* The RX thread's ring choice (reference src/rx_pcap.c:19-25,67-80) for a batch resident in GPU
 * memory ("Batch layout", the UPE_FRAME_TAIL rule of upe_gpu_process), `rings` a power of two up
 * to UPE_RX_RINGS_MAX: a packet whose parse_flow_key succeeds (src/parser.c:6-111) goes to ring
 * flow_hash & (rings - 1) (src/parser.c:113-135); every other packet — ARP and ICMPv6 NS/NA
 * among them, the RX thread does not call handle_control_packet — goes to the ring named by the
 * round-robin cursor, which then steps: the k-th such packet of the batch (k from 0) to ring
 * (rr_start + k) & (rings - 1).  Each ring receives its packets in arrival order.  Uses no rule
 * or neighbour table and writes nothing to the frames.
 *   d_ring[i]      packet i's ring, | UPE_RX_FALLBACK when the cursor chose it
 *   d_flow_hash[i] optional: flow_hash of a parsed packet, 0 otherwise
 *   d_index        the stable partition by ring: ring r's packets, ascending, are
 *                  d_index[start_r .. start_r + d_counts[r]), start_r = d_counts[0] + ... +
 *                  d_counts[r - 1]
 *   d_desc_out     optional: d_desc_out[k] = d_desc[d_index[k]]
 *   d_counts       rings + 1 entries: packets per ring, then the number of fallback packets
 * d_desc_out + start_r is a ready descriptor array of d_counts[r] packets over the same
 * d_frames: worker r is then a context of its own (its own L1 caches, counters and rule_stats,
 * as one reference worker_t, src/main.c:444-456) calling upe_gpu_process* on that segment.  Rings
 * hold disjoint packets, so the workers' in-place rewrites do not collide.
 * The cursor for the next batch is (rr_start + d_counts[rings]) & (rings - 1); the caller carries
 * it, as the reference's `static rr` does (rr_start is taken & (rings - 1)).
 * Asynchronous on `stream` like upe_gpu_process (three launches; scratch lives in the context,
 * so a context's dispatches are queued one after another).  n == 0 zeroes d_counts and launches
 * nothing.  -1 before any launch: rings 0, not a power of two or above UPE_RX_RINGS_MAX; a NULL
 * required buffer with n > 0 (d_counts always); n beyond the kernels' 32-bit indexes.
 * Out of scope, host ring mechanics: the drop of packets a full ring refuses
 * (src/rx_pcap.c:31-36) and the 32-packet staging bursts (src/rx_pcap.c:80-92).
 * UPE_RX_BLOCK: packets per workgroup of the dispatch kernels (batch sizes around it are where
 * tests look). */
#define UPE_RX_RINGS_MAX 64
#define UPE_RX_FALLBACK 0x80000000u
#define UPE_RX_BLOCK 1024
int upe_gpu_rx_dispatch(upe_gpu_ctx_t *ctx, const uint8_t *d_frames, const uint64_t *d_desc,
                        size_t n, uint32_t rings, uint32_t rr_start,
                        uint32_t *d_ring,      /* n */
                        uint32_t *d_flow_hash, /* n, optional */
                        uint32_t *d_index,     /* n */
                        uint64_t *d_desc_out,  /* n, optional */
                        uint64_t *d_counts,    /* rings + 1 */
                        void *stream);

/* Egress list: d_index[0..*d_count) = the indexes i < n whose verdict code is `code` (e.g.
 * UPE_V_FWD), in packet order — the order process_packet queues frames for tx_send_batch
 * (reference src/worker.c:240-243, 287-303).  Device buffers; d_index holds n entries. */
int upe_gpu_compact(upe_gpu_ctx_t *ctx, const uint32_t *d_verdict, size_t n, uint32_t code,
                    uint32_t *d_index, uint64_t *d_count, void *stream);

/* upe_gpu_process_emit() plus the egress list in the same pass, with no second kernel (round 6):
 * the forwarded packets of group g (packets 64g .. 64g + 63) are d_tx[64g .. 64g + d_tx_count[g])
 * in packet order — the order process_packet queues frames for tx_send_batch (reference
 * src/worker.c:240-243, 287-303) — and d_tx[64g + k] is the packet whose record is d_hdr[64g + k]
 * (the records' UPE_HDR_SLOT layout).  The groups concatenated are exactly upe_gpu_compact(...,
 * UPE_V_FWD, ...)'s list; upe_tx_flush_groups() makes the reference worker's TX calls from it
 * directly.  Device buffers: d_tx holds n entries, d_tx_count (n + 63) / 64; slots past a group's
 * count are not written.  0 / -1. */
int upe_gpu_process_emit_tx(upe_gpu_ctx_t *ctx, uint8_t *d_frames, const uint64_t *d_desc,
                            uint32_t *d_verdict, upe_hdr_rec_t *d_hdr, uint32_t *d_tx,
                            uint32_t *d_tx_count, size_t n, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Egress batch: the forwarded frames packed back to back on the device                        */
/* ------------------------------------------------------------------------------------------ */
/* The bytes that go out, for a classified batch resident in GPU memory: the frames process_packet
 * queues for tx_send_batch (reference src/worker.c:240-243), rewritten exactly as it leaves them
 * in b->data (src/worker.c:162-244), in the order it queues them (src/worker.c:287-303), back to
 * back in d_out.  The output is itself a "Batch layout" with its own descriptors: a TX path
 * copies back (or DMAs) only the forwarded bytes, in one piece; a next stage classifies it as its
 * input batch; upe_tx_flush_packed makes the reference worker's TX calls from it.
 *
 * Packing rule.  Let f_0 < f_1 < ... be the packets whose verdict code is UPE_V_FWD (only the code
 * of a verdict word is read) and len_k the length in d_desc[f_k].  Packed frame k starts at
 * o_k = the sum over j < k of (len_j + 15) & ~15, and
 *   d_out_desc[k]  = UPE_DESC(o_k, len_k)
 *   d_out_index[k] = f_k                              (optional)
 *   d_out[o_k .. o_k + len_k) = the frame; the bytes up to the next 16-byte boundary are zero,
 *                    so every byte of [0, bytes) is defined.
 * The frame bytes are, with d_hdr == NULL, a copy of the frame (the batch went through
 * upe_gpu_process, _rss or _segmented, which rewrote it in place); with d_hdr, the untouched
 * frame with its record applied byte for byte as upe_hdr_apply does (the batch went through
 * upe_gpu_process_emit, _emit_tx, _ring_emit or _queue_emit).  Packet i's record is found by the
 * UPE_HDR_SLOT rule, slot 64 * (i / 64) + its rank among the forwarded packets of its 64-group;
 * rec[i] is never read.  A patched byte position at or beyond len is not written.
 *
 * Capacity.  Frame k is packed only if o_k + ((len_k + 15) & ~15) <= out_bytes; offsets ascend,
 * so the packed frames are a prefix, counted in `packed`; `need` is the size to retry with.
 * Nothing at or beyond d_out + out_bytes is written, and entries of d_out_desc / d_out_index
 * from `packed` on are not written.
 *
 * Not done here: the UPE_FRAME_TAIL bytes after the last frame are not written (a caller that
 * feeds d_out to another classify sizes it for them, as for any batch).  The call needs FULL
 * frames, as upe_gpu_process_segmented does: a batch of header windows (UPE_HDR_WINDOW) is not
 * valid input, the bytes past a window would be packed as payload.  Frames are read in whole
 * 16-byte quads (the quad holding a frame's last byte is read whole, never a quad past it).  ARP
 * requests answered in place (UPE_VF_ARP_REPLY, code DROP_PARSE) are not in the output: the
 * reference sends those at once through tx_send, outside the batch queue (src/worker.c:40-52).
 *
 * Asynchronous on `stream` (three launches; scratch lives in the context, so a context's packs
 * are queued one after another).  n == 0 zeroes *d_info and launches nothing.  -1 before any
 * launch: a NULL required pointer with n > 0 (d_info always); d_out not 16-byte aligned; n beyond
 * the kernels' 32-bit indexes; d_out overlapping d_frames in address — the call cannot see where
 * the frames end, so d_frames counts up to the end of the device allocation that holds it (a
 * caller carving both out of one allocation puts d_out below d_frames).
 * UPE_EGRESS_BLOCK: packets per workgroup of the pack kernels (batch sizes around it are where
 * tests look). */
#define UPE_EGRESS_BLOCK 1024
typedef struct {
    uint64_t frames; /* forwarded packets in the batch */
    uint64_t packed; /* of those, written to d_out (a prefix in packet order) */
    uint64_t bytes;  /* bytes of d_out used by the packed frames, padding included */
    uint64_t need;   /* bytes all `frames` would use (== bytes when everything fitted) */
} upe_egress_info_t;
int upe_gpu_egress_pack(upe_gpu_ctx_t *ctx, const uint8_t *d_frames, const uint64_t *d_desc,
                        const uint32_t *d_verdict,
                        const upe_hdr_rec_t *d_hdr, /* NULL: frames were rewritten in place */
                        size_t n,
                        uint8_t *d_out, size_t out_bytes,
                        uint64_t *d_out_desc,       /* n */
                        uint32_t *d_out_index,      /* n, optional */
                        upe_egress_info_t *d_info,  /* device, 32 bytes */
                        void *stream);

/* The reference worker's TX calls (src/worker.c:287-303) from a packed egress batch copied to the
 * host (h_out[0 .. info.bytes), h_out_desc, h_out_index, count = info.packed): the same calls,
 * arguments and accounting as upe_tx_flush over the classified ingress batch — one `send` per
 * input burst (h_out_index[k] / burst) that forwarded anything, at most UPE_TX_BATCH_MAX frames
 * per call — with the frame pointers pointing into h_out; the ingress buffer is not needed.  All
 * arguments are checked before the first `send`: -1, with no call made, for a burst of 0 or above
 * UPE_TX_BATCH_MAX, a NULL argument with count > 0, or an index list that does not ascend
 * strictly. */
int upe_tx_flush_packed(const uint8_t *h_out, const uint64_t *h_out_desc,
                        const uint32_t *h_out_index, size_t count, size_t burst,
                        upe_tx_batch_fn send, void *user, uint64_t *forwarded, uint64_t *dropped);

/* A batch with exact control-packet semantics, as the reference's burst loop runs it
 * (src/worker.c:23-104 inside process_packet): an ARP packet with the Ethernet/IPv4 header, or
 * an NDP NS/NA carrying a link-layer address option, writes a neighbour table, and every later
 * packet sees the new entry.  The batch is cut after each such packet: the segment up to and
 * including it runs as upe_gpu_process(), its write — arp_update(spa, sha)
 * (src/arp_table.c:26-53) or ndp_update(src | target, lladdr) (src/ndp_table.c:39-65, option
 * walk src/worker.c:68-95) — is applied to the caller's host slot arrays `arp` / `ndp` (the
 * ones last given to upe_gpu_load_neigh; updated in place, update_at = now, as the reference's
 * tables are), the new snapshot is uploaded, and the next segment runs.  Control packets are
 * found on the device (one marking pass plus an ordered compaction), so a batch without them
 * costs one extra pass.  Synchronous; *n_writes (optional) = table writes applied.  Capacities
 * are powers of two, as arp_table_init / ndp_table_init require.  The NS/NA option walk reads
 * the whole frame (len bytes), so this call needs FULL frames: a batch of UPE_FRAME_TAIL-byte
 * header windows (upe_gpu_process_host's window form) is not valid here — an NS/NA longer than
 * its window would have its options read from the bytes that follow the window.  When the
 * upe_gpu_load_neigh of a table write fails, the call (and upe_gpu_process_segmented_resident)
 * returns -1 with that call's message and the snapshot loaded before the write stays loaded;
 * nothing is promised about the outputs of the partly processed batch. */
int upe_gpu_process_segmented(upe_gpu_ctx_t *ctx, uint8_t *d_frames, const uint64_t *d_desc,
                              uint32_t *d_verdict, size_t n, upe_arp_entry_t *arp,
                              size_t arp_capacity, upe_ndp_entry_t *ndp, size_t ndp_capacity,
                              int64_t now, size_t *n_writes, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Control writes: what a resident batch's control packets teach, as records                   */
/* ------------------------------------------------------------------------------------------ */
/* The table writes of handle_control_packet (reference src/worker.c:23-104) for a batch resident
 * in GPU memory ("Batch layout", the UPE_FRAME_TAIL rule of upe_gpu_process), without the host
 * touching a frame byte: one 32-byte record per arp_update / ndp_update the reference would call,
 * in packet order.  Frames are read only; a byte at or past len reads as zero and never
 * influences a result.  The batch holds FULL frames, as for upe_gpu_process_segmented: the NS / NA
 * option walk reads up to len bytes of a frame.
 *
 * Marked packets: the rule upe_gpu_ingress_gather documents for d_ctrl (ctrl_table_write,
 * csrc/upe_dev.h); info.ctrl counts them.
 * ARP (src/worker.c:28-39): a marked ARP packet always yields a record — arp_update(ntohl(spa),
 * sha).  The learn does not look at len: spa and sha bytes at or past len are zero.  The reply
 * (src/worker.c:40-52), the port address and op play no part.
 * NS / NA (src/worker.c:57-95): off = 78; while off + 2 <= len: ot = f[off], ol =
 * (uint8_t)(f[off + 1] * 8) — the reference's uint8_t opt_len: a length byte of 32 wraps to 0, 33
 * to 8; stop if ol == 0 or off + ol > len; a record — ndp_update(NS: the IPv6 source, NA: the
 * target; mac = f[off + 2 .. off + 8)) — if (NS and ot == 1) or (NA and ot == 2); else off += ol.
 * An NS / NA with no such option yields no record (it is still counted in ctrl).
 * The records do not depend on any table: whether a table exists, or is full, is decided when
 * they are applied (upe_neigh_apply_writes).
 *
 * d_writes[0 .. stored) are the records in ascending index, stored = min(writes, cap); nothing at
 * or past d_writes + cap is written, and `writes` is the cap to retry with.  Asynchronous on
 * `stream` (NULL: the context's), at most three launches; scratch lives in the context, so a
 * context's calls are queued one after another.  Otherwise read-only with respect to the context:
 * tables, counters, rule_stats, the L1 state, the latency histogram and upe_gpu_launch_info are
 * untouched and no launch is counted.  n == 0 zeroes *d_info with first_write = UINT64_MAX and
 * launches nothing.  -1 (upe_gpu_last_error()) before any launch: a NULL context; NULL d_frames or
 * d_desc with n > 0; a NULL d_info; a NULL d_writes with cap > 0; d_writes not 16-byte aligned; n
 * above 2^32 - 1 - UPE_CTRL_BLOCK.
 * UPE_CTRL_BLOCK: packets per workgroup of the kernels (batch sizes around it are where tests
 * look). */
#define UPE_CTRL_BLOCK 1024
enum { UPE_CW_ARP = 4, UPE_CW_NDP = 6 };
typedef struct {        /* 32 bytes, every byte written */
    uint32_t index;     /* packet position in the batch */
    uint8_t kind;       /* UPE_CW_ARP: arp_update; UPE_CW_NDP: ndp_update */
    uint8_t zero0;
    uint16_t mac_off;   /* frame offset the MAC was read from: 22 (ARP sha), or the chosen
                           option's offset + 2 (NDP) */
    uint8_t mac[6];
    uint16_t zero1;
    uint8_t ip[16];     /* ARP: bytes 0-3 = ntohl(spa) as a little-endian word (upe_ip_addr_t.v4),
                           bytes 4-15 zero.  NDP: the 16 wire bytes (NS: the IPv6 source, frame
                           bytes 22..37; NA: the target, frame bytes 62..77) */
} upe_ctrl_write_t;
typedef struct {          /* device, 32 bytes */
    uint64_t ctrl;        /* packets the marking rule selects (== ingress_gather's n_ctrl) */
    uint64_t writes;      /* records the batch has */
    uint64_t stored;      /* min(writes, cap): a prefix in packet order */
    uint64_t first_write; /* index of the first record's packet, or UINT64_MAX */
} upe_ctrl_info_t;

int upe_gpu_ctrl_writes(upe_gpu_ctx_t *ctx, const uint8_t *d_frames, const uint64_t *d_desc,
                        size_t n, upe_ctrl_write_t *d_writes, size_t cap,
                        upe_ctrl_info_t *d_info, void *stream);

/* upe_gpu_ctrl_writes' exact host twin (upe_host.c): the same bytes in writes[0 .. stored) and
 * *info for a batch in host memory.  No GPU needed.  0 / -1 (upe_host_last_error()): NULL frames
 * or desc with n > 0, a NULL info, NULL writes with cap > 0, n above 2^32 - 1 - UPE_CTRL_BLOCK. */
int upe_ctrl_writes_host(const uint8_t *frames, const uint64_t *desc, size_t n,
                         upe_ctrl_write_t *writes, size_t cap, upe_ctrl_info_t *info);

/* The records applied, in order, to the caller's slot arrays: arp_update (src/arp_table.c:26-53:
 * from slot ip & (capacity - 1), the first slot that is free or holds the address, at most
 * capacity probes) and ndp_update (src/ndp_table.c:39-65, from hash_ipv6 :6-17), update_at = now
 * on every slot written; a full table with no matching slot is left alone.  *applied (optional) =
 * the records whose family has a table (capacity > 0): what upe_gpu_process_segmented counts in
 * n_writes.  Capacities are powers of two, or NULL with capacity 0.  Everything is checked before
 * the first write: -1 (upe_host_last_error()), with nothing changed, for a bad capacity, a missing
 * table, NULL writes with count > 0, or a record whose kind is neither UPE_CW_ARP nor UPE_CW_NDP.
 * The caller then uploads the tables (upe_gpu_load_neigh). */
int upe_neigh_apply_writes(upe_arp_entry_t *arp, size_t arp_capacity,
                           upe_ndp_entry_t *ndp, size_t ndp_capacity,
                           const upe_ctrl_write_t *writes, size_t count, int64_t now,
                           size_t *applied);

/* The records applied to the LOADED snapshot, on the device, where that moves nothing
 * (csrc/upe_neigh_patch.hip): a refresh — a record whose address the snapshot already holds —
 * rewrites the MAC of the one index slot a lookup of that address answers from, as arp_update /
 * ndp_update rewrite the slot their probe, which is the lookup's, arrives at (src/arp_table.c:26-80,
 * src/ndp_table.c:39-86).  No index is rebuilt and nothing is uploaded.
 * Address held: a UPE_CW_ARP record's when arp_get_mac of ip bytes 0-3 (the little-endian word)
 * hits in the loaded snapshot, a UPE_CW_NDP record's when ndp_get_mac of the 16 bytes does — the
 * answers upe_gpu_resolve_keys gives before the call.
 * Result: the snapshot after the call is the snapshot before it with the held records applied in
 * rank order (rank: position in d_writes): of the held records aimed at one slot the one of
 * highest rank supplies the six MAC bytes; the slot's address, its used bit and every slot no
 * record aims at keep every bit.
 * Missed records: a record whose address is not held — a new neighbour, a family whose index is
 * empty, a kind that is neither UPE_CW_ARP nor UPE_CW_NDP — changes nothing.  d_miss[0 .. missed)
 * (optional) are their ranks, ascending; nothing at or past d_miss + missed is written; patched +
 * missed == records.  The caller applies them on the host, in order (upe_neigh_apply_writes, then
 * upe_gpu_load_neigh); applying every held record here and the missed ones there gives the
 * reference's tables (DESIGN.md §3 has the argument).
 * Derived state: what a snapshot load does to the context after its swap happens after a patch
 * too, on `stream`: whether the L1 entries still agree with the tables is asked again.  The L1
 * entries themselves are not touched (the reference never invalidates last_arp_ip / last_ndp_ip: a
 * packet aimed at an L1 entry keeps getting the old MAC).
 * Asynchronous on `stream` (NULL: the context's) and ordered like a launch: a classify queued
 * before the call reads the old MACs, one queued after it the new ones.  Three launches of its
 * own, then the one or two of the derived state; scratch lives in the context.  Counters,
 * rule_stats, the latency histogram, upe_gpu_launch_info and any upe_neigh_image_t the caller
 * holds are untouched (an image is a value: the context's device copy alone changes), and no
 * launch is counted.  count == 0 zeroes *d_info with first_miss = UINT64_MAX and launches
 * nothing.  -1 (upe_gpu_last_error()) before any launch: a NULL context; a NULL d_info; a NULL
 * d_writes with count > 0; d_writes not 16-byte aligned; count above 2^32 - 1 - UPE_PATCH_BLOCK.
 * UPE_PATCH_BLOCK: records per workgroup of the kernels (counts around it are where tests look). */
#define UPE_PATCH_BLOCK 256
typedef struct {          /* device, 32 bytes, every byte written */
    uint64_t records;     /* count */
    uint64_t patched;     /* records whose address the loaded snapshot holds */
    uint64_t missed;      /* the rest */
    uint64_t first_miss;  /* rank of the first missed record, or UINT64_MAX */
} upe_neigh_patch_info_t;

int upe_gpu_neigh_patch(upe_gpu_ctx_t *ctx, const upe_ctrl_write_t *d_writes, size_t count,
                        uint32_t *d_miss /* count entries, optional */,
                        upe_neigh_patch_info_t *d_info, void *stream);

/* upe_gpu_neigh_patch's exact host twin (csrc/upe_rules.cpp) on a compiled snapshot
 * (upe_neigh_compile): the same change to the image, the same bytes in miss[0 .. missed) and
 * *info.  No GPU needed.  0 / -1 (upe_gpu_last_error()): a NULL image or info, NULL writes with
 * count > 0, count above 2^32 - 1 - UPE_PATCH_BLOCK.
 * upe_neigh_image_lookup_host: what a context that has loaded the image answers
 * (upe_gpu_resolve_keys' format and rules), by the index's own three-slot lookup. */
int upe_neigh_patch_host(upe_neigh_image_t *image, const upe_ctrl_write_t *writes, size_t count,
                         uint32_t *miss /* count entries, optional */,
                         upe_neigh_patch_info_t *info);
int upe_neigh_image_lookup_host(const upe_neigh_image_t *image, const upe_flow_key_t *keys,
                                size_t n, uint64_t *mac);

/* New neighbours learnt on the device (csrc/upe_neigh_learn.hip): the records applied to the LOADED
 * snapshot, the ones for an address it does not hold included — arp_update (src/arp_table.c:26-53)
 * and ndp_update (src/ndp_table.c:39-65) of a new address take the first free slot of the probe,
 * which exists whenever the table has an invalid slot and every valid entry is one a probe
 * reaches; the lookups of such a table do not depend on where in the index an entry lies, so the
 * address may take any free candidate slot of the index (DESIGN.md §3 has the argument).
 *
 * What a snapshot carries for this, per family, from the slot array it was compiled from
 * (upe_neigh_image_read): free — the invalid slots; insertable — every valid slot is one a probe
 * reaches and the index has slots (bits != 0).  A context keeps the two free counts on the device
 * beside the index; a learn counts them down, a load sets them.
 * upe_neigh_compile_room: upe_neigh_compile with each index sized for its reachable addresses plus
 * `room` more (the placement starts at 2^bits * 4 >= (n + room) * 5), so that a burst of new
 * addresses finds free candidate slots; a family without reachable addresses and room > 0 gets a
 * real index with no slot used.  room 0 / 0 gives upe_neigh_compile's image byte for byte.  NULL
 * on error, as there; also for a room above 2^30.
 *
 * The result is that of this loop over the records in rank order (rank: position in d_writes),
 * on the loaded index and free[family]:
 *   1. a kind that is neither UPE_CW_ARP nor UPE_CW_NDP: deferred;
 *   2. the address is held now (the index's own lookup hits): the six MAC bytes of the slot that
 *      answers are rewritten — patched;
 *   3. else the family is not insertable: deferred;
 *   4. else free == 0: dropped (the reference's full table does nothing);
 *   5. else the first of slot1, slot2, slot3 (csrc/upe_dev.h) whose used bit is clear takes the
 *      address, the MAC and the used bit; free-- — inserted;
 *   6. else (no candidate slot is free): deferred, free unchanged.
 * d_defer[0 .. deferred) (optional) are the deferred ranks, ascending; nothing at or past d_defer +
 * deferred is written; patched + inserted + dropped + deferred == records.  After a call with
 * deferred > 0 the caller applies the records on the host and loads (upe_neigh_apply_writes, then
 * upe_gpu_load_neigh), as after a patch's misses; the load supersedes the device state.  bits, seed
 * and every slot no record is aimed at keep every bit; no index is rebuilt, nothing is uploaded.
 * Stream order, derived state (the L1 entries stay; their agreement with the tables is asked
 * again), counters and launch info: upe_gpu_neigh_patch's rules — nothing is counted.  One launch
 * of its own: one workgroup takes UPE_LEARN_CHUNK records per step, in rank order, so no result
 * depends on how workgroups are scheduled; then the launches of the derived state.
 * count == 0 zeroes *d_info with first_defer = UINT64_MAX and launches nothing.  -1
 * (upe_gpu_last_error()) before any launch: a NULL context; a NULL d_info; a NULL d_writes with
 * count > 0; d_writes not 16-byte aligned; count above 2^32 - 1 - UPE_LEARN_CHUNK.
 * UPE_LEARN_CHUNK: records per step (counts around it are where tests look). */
#define UPE_LEARN_CHUNK 1024
typedef struct {          /* device, 64 bytes, every byte written */
    uint64_t records;     /* count */
    uint64_t patched;     /* records that took step 2 */
    uint64_t inserted;    /* records that took step 5 */
    uint64_t dropped;     /* records that took step 4 */
    uint64_t deferred;    /* records that took step 1, 3 or 6 */
    uint64_t first_defer; /* rank of the first deferred record, or UINT64_MAX */
    uint64_t arp_free;    /* free of the ARP family after the call */
    uint64_t ndp_free;    /* free of the NDP family after the call */
} upe_neigh_learn_info_t;
typedef struct {          /* host, 32 bytes */
    uint32_t arp_bits, arp_seed, ndp_bits, ndp_seed;   /* the indexes: 2^bits slots, 0 = none */
    uint32_t arp_free, ndp_free;                       /* invalid slots of the compiled arrays */
    uint32_t arp_insertable, ndp_insertable;           /* 0 / 1 */
} upe_neigh_image_info_t;

upe_neigh_image_t *upe_neigh_compile_room(const upe_arp_entry_t *arp, size_t arp_capacity,
                                          const upe_ndp_entry_t *ndp, size_t ndp_capacity,
                                          size_t arp_room, size_t ndp_room);
int upe_gpu_neigh_learn(upe_gpu_ctx_t *ctx, const upe_ctrl_write_t *d_writes, size_t count,
                        uint32_t *d_defer /* count entries, optional */,
                        upe_neigh_learn_info_t *d_info, void *stream);

/* upe_gpu_neigh_learn's exact host twin (csrc/upe_rules.cpp): the loop above, written out, on a
 * compiled snapshot — the same index bytes and free counts in the image, the same bytes in
 * defer[0 .. deferred) and *info (arp_update: src/arp_table.c:26-53, ndp_update:
 * src/ndp_table.c:39-65).  No GPU needed.  0 / -1 (upe_gpu_last_error()): a NULL image or info,
 * NULL writes with count > 0, count above 2^32 - 1 - UPE_LEARN_CHUNK.
 * upe_neigh_image_read: what an image holds — *info (optional), and the index slot arrays into arp
 * / ndp (each optional; 16 bytes per ARP slot, 32 per NDP slot, 2^bits slots, one zero slot where
 * bits == 0), each copied only when its size in bytes is given exactly; -1 otherwise. */
int upe_neigh_learn_host(upe_neigh_image_t *image, const upe_ctrl_write_t *writes, size_t count,
                         uint32_t *defer /* count entries, optional */,
                         upe_neigh_learn_info_t *info);
int upe_neigh_image_read(const upe_neigh_image_t *image, upe_neigh_image_info_t *info,
                         void *arp, size_t arp_bytes, void *ndp, size_t ndp_bytes);

/* upe_gpu_process_segmented without a frame byte on the host (csrc/upe_segment.hip): the same
 * batch, arguments and outputs, bit for bit — verdict words, frames, counters, rule_stats, the L1
 * state and the caller's slot arrays (update_at included).  The batch's records come from
 * upe_gpu_ctrl_writes (one copy of its info and records to the host, one synchronisation); the
 * batch is cut after every marked packet, as there (when some marked packet has no record, their
 * positions are listed on the device first, one more small copy); for each record, in order, the
 * segment up to and including its packet is queued, the record is
 * applied to the host arrays (upe_neigh_apply_writes), and the device follows: a record whose
 * address the arrays held (upe_neigh_lookup_host, before the write) is queued as a
 * upe_gpu_neigh_patch of that one record — no synchronisation, no rebuild — and any other takes
 * upe_gpu_load_neigh.  A record whose family has no table (capacity 0) is skipped, as there.
 * Synchronous at return.  A batch without records costs the upe_gpu_ctrl_writes pass and one
 * classify.  info (optional): writes = upe_gpu_process_segmented's *n_writes; patched + rebuilds
 * == writes; ctrl = the marked packets. */
typedef struct { uint64_t writes, patched, rebuilds, ctrl; } upe_segment_info_t;   /* host */
int upe_gpu_process_segmented_resident(upe_gpu_ctx_t *ctx, uint8_t *d_frames,
                                       const uint64_t *d_desc, uint32_t *d_verdict, size_t n,
                                       upe_arp_entry_t *arp, size_t arp_capacity,
                                       upe_ndp_entry_t *ndp, size_t ndp_capacity, int64_t now,
                                       upe_segment_info_t *info, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Release order: what happens to every buffer of a classified batch afterwards               */
/* ------------------------------------------------------------------------------------------ */
/* worker_main (reference src/worker.c:280-303) frees the buffer of a dropped or consumed packet
 * at that packet's exit from process_packet, in packet order (src/worker.c:97, 123, 135, 151, 170,
 * 209, 252), queues a forwarded packet's buffer in tx_bufs[] (src/worker.c:240-243) and frees the
 * queue, in queue order, after the burst's tx_send_batch (src/worker.c:287-303); an ARP request it
 * answers goes out through tx_send before its buffer is freed (src/worker.c:51, then :123).  The
 * reference pool is a LIFO stack behind a thread-local cache (src/pktbuf.c), so the order of the
 * frees is the order of every later pktbuf_alloc.  upe_gpu_release_order builds that order for a
 * classified batch resident in GPU memory (csrc/upe_release.hip); upe_release_flush makes the
 * reference's calls from the lists, without looking at a verdict word.
 *
 * Bursts: either a fixed size (d_burst_first == NULL: burst b is packets [b * burst, min((b + 1) *
 * burst, n)), 1 <= burst <= UPE_TX_BATCH_MAX, nb ignored; the form upe_tx_flush takes), or an
 * offset array on the device (d_burst_first[0 .. nb]: burst b is [first[b], first[b + 1])), for a
 * worker whose ring pops vary in size.  The array is valid when first[0] == 0, first[nb] == n and
 * every burst holds 1 to UPE_TX_BATCH_MAX packets.  info.bad_bursts counts the violated conditions:
 * one for first[0] != 0, one for first[nb] != n, one per burst b whose first[b + 1] - first[b]
 * (modulo 2^32) is not in 1 .. UPE_TX_BATCH_MAX.  When it is nonzero *d_info is still written in
 * full (the counts over the verdicts do not depend on bursts) and NO other output is touched; the
 * call cannot see a device array before launching, so this is not a return value.
 *
 * Order.  For burst b = [s, e) with r packets whose verdict code is not UPE_V_FWD:
 *   d_order[s .. s + r)   those packets' positions, ascending: process_packet's frees
 *   d_order[s + r .. e)   the forwarded packets' positions, ascending: tx_bufs[], which is the
 *                         burst's tx_send_batch argument order and the frees after it
 *   d_burst_fwd[b]        e - s - r
 *   d_handle[k]           d_slot[d_order[k]] (both given, or neither)
 *   d_reply[0 .. replies) the positions whose verdict has UPE_VF_ARP_REPLY, ascending over the
 *                         whole batch; nothing at or past d_reply + replies is written
 * Only the code of a verdict word decides forwarded / consumed / dropped and only the flag bit
 * decides reply: hand-made words are valid input, as for upe_gpu_compact.  The forwarded ranges of
 * d_order, concatenated over the bursts, are exactly upe_gpu_compact(..., UPE_V_FWD, ...)'s list.
 *
 * Asynchronous on `stream` (NULL: the context's), ordered like a launch, at most three launches;
 * scratch lives in the context, so a context's calls are queued one after another.  Counters, rule_stats,
 * the latency histogram, the tables and upe_gpu_launch_info are untouched and no launch is counted.
 * n == 0 zeroes *d_info with first_reply = UINT64_MAX and launches nothing.  -1
 * (upe_gpu_last_error()) before any launch: a NULL context or d_info; NULL d_verdict, d_order or
 * d_burst_fwd with n > 0; exactly one of d_slot / d_handle; d_burst_first == NULL with burst 0 or
 * above UPE_TX_BATCH_MAX; d_burst_first given with nb == 0 && n > 0 or nb > n; n above 2^32 - 1 -
 * UPE_RELEASE_BLOCK.
 * UPE_RELEASE_BLOCK: packets per workgroup of the kernels (batch sizes around it are where tests
 * look). */
#define UPE_RELEASE_BLOCK 1024
typedef struct {            /* device, 64 bytes, every byte written */
    uint64_t packets;       /* n */
    uint64_t bursts;        /* nb, or ceil(n / burst) in the fixed form */
    uint64_t forwarded;     /* verdict code UPE_V_FWD */
    uint64_t consumed;      /* code UPE_V_CONSUMED */
    uint64_t dropped;       /* every other code */
    uint64_t replies;       /* UPE_VF_ARP_REPLY set */
    uint64_t first_reply;   /* position of the first, or UINT64_MAX */
    uint64_t bad_bursts;    /* violated conditions of the offset array (0 in the fixed form) */
} upe_release_info_t;

int upe_gpu_release_order(upe_gpu_ctx_t *ctx, const uint32_t *d_verdict, size_t n,
                          const uint32_t *d_burst_first, /* nb + 1 offsets, or NULL */
                          size_t nb, uint32_t burst,     /* with NULL: fixed size, nb ignored */
                          const uint32_t *d_slot,        /* n handles, optional */
                          uint32_t *d_order,             /* n */
                          uint32_t *d_handle,            /* n; given iff d_slot is */
                          uint32_t *d_burst_fwd,         /* one per burst */
                          uint32_t *d_reply,             /* n, optional */
                          upe_release_info_t *d_info, void *stream);

/* upe_gpu_release_order's exact host twin (upe_host.c): the same arguments on host arrays, the
 * same bytes in order, handle, burst_fwd, reply[0 .. replies) and *info, nothing else written when
 * bad_bursts is nonzero.  No GPU needed.  0 / -1 (upe_host_last_error()) for the same arguments. */
int upe_release_order_host(const uint32_t *verdict, size_t n, const uint32_t *burst_first,
                           size_t nb, uint32_t burst, const uint32_t *slot, uint32_t *order,
                           uint32_t *handle, uint32_t *burst_fwd, uint32_t *reply,
                           upe_release_info_t *info);

/* The reference worker's calls from those lists, copied to the host.  Per burst b = [s, e), in
 * order, with f = h_burst_fwd[b] and r = e - s - f:
 *   1. send_one(frame, len) for each reply position inside the burst, ascending;
 *   2. release(handles of h_order[s .. s + r)) in one call, skipped when r == 0;
 *   3. when f > 0: one send() of the frames of h_order[s + r .. e) (pointers h_frames + offset,
 *      lengths from h_desc; arguments and accounting as upe_tx_flush), then release() of their
 *      handles.
 * A handle is h_handle[k], or h_order[k] itself when h_handle is NULL.  release() stands for
 * pktbuf_free of each handle in the order given.
 * The one regrouping against the reference: a reply's tx_send moves ahead of the frees of the
 * earlier packets of its burst.  It stays before its own buffer's free and before the burst's
 * tx_send_batch, and the sequence of frees and the sequence of sends are each the reference's own.
 * Everything is checked before the first callback (all or nothing): -1 (upe_host_last_error())
 * with no call made for a NULL argument that is needed, a bad burst description (a fixed size of 0
 * or above UPE_TX_BATCH_MAX; an offset array that is not valid, nb == 0 with n > 0, nb > n), an
 * h_burst_fwd[b] above its burst's size, an h_order entry outside its burst, or a reply list that
 * does not ascend strictly or names a position >= n. */
typedef struct {
    int  (*send_one)(void *user, const uint8_t *frame, size_t len);      /* tx_send */
    upe_tx_batch_fn send;                                                /* tx_send_batch */
    void (*release)(void *user, const uint32_t *handles, size_t count);  /* pktbuf_free of each */
} upe_release_ops_t;
int upe_release_flush(const uint8_t *h_frames, const uint64_t *h_desc, const uint32_t *h_order,
                      const uint32_t *h_handle /* NULL: h_order's values are the handles */,
                      const uint32_t *h_burst_first, size_t nb, uint32_t burst, size_t n,
                      const uint32_t *h_burst_fwd, const uint32_t *h_reply, size_t replies,
                      const upe_release_ops_t *ops, void *user,
                      uint64_t *forwarded, uint64_t *dropped);

/* Wait for all work queued on the context's stream (or `stream`). */
int upe_gpu_sync(upe_gpu_ctx_t *ctx, void *stream);

/* Summary of the most recent upe_gpu_process() (synchronises). */
int upe_gpu_batch_info(upe_gpu_ctx_t *ctx, upe_batch_info_t *info);

/* How the most recent classify launch ran (synchronises; diagnostics and tests).  A launch that
 * starts from an L1 entry disagreeing with its table resolves the packets aimed at that entry by
 * a bounded look-back; a wave that stops waiting (a workgroup it needs is not resident yet)
 * defers them, and the launch's last workgroup answers them. */
typedef struct {
    uint32_t variant;  /* kernel variant: bit 0 emit, 1 tuple space, 2 lean, 3 no look-back,
                          4 ring (stamped), 5 a host path (upe_gpu_process_mapped / _host),
                          6-7 a two-bit field, how a linear-scan table is matched: 0 small table
                          (up to 64 rules), 1 per-family rule lists, 2 the whole table scanned,
                          3 the decision tree over the family lists */
    uint32_t grid;     /* workgroups of the launch */
    uint32_t deferred; /* (chunk, family) entries whose look-back was deferred to the last
                          workgroup (0 when the look-back was not live) */
    uint64_t launches; /* classify launches of this context so far */
} upe_launch_info_t;
int upe_gpu_launch_info(upe_gpu_ctx_t *ctx, upe_launch_info_t *info);

/* Accumulated worker counters and rule_stats[0..capacity) (synchronises). */
int upe_gpu_get_stats(upe_gpu_ctx_t *ctx, upe_counters_t *counters, upe_rule_stat_t *rule_stats,
                      size_t capacity);
int upe_gpu_reset_stats(upe_gpu_ctx_t *ctx);

/* ------------------------------------------------------------------------------------------ */
/* Latency histogram: the worker's per-packet dataplane latency                                */
/* ------------------------------------------------------------------------------------------ */
/* The fourth output of worker_t the reference's stats thread reads (src/main.c:284-351, the
 * "Dataplane latency" block): latency_hist, sampled at every exit of process_packet that frees or
 * queues a buffer (src/worker.c:120-122, 132-134, 148-150, 167-169, 206-208, 235-237, 249-251),
 * not at the early return for an NDP NS/NA that handle_control_packet consumed
 * (src/worker.c:111).
 *
 * The histogram (mirrors latency_histogram_t, reference include/latency.h:21-40, 96 bytes): eight
 * buckets with the upper bounds UPE_LATENCY_BOUNDS (ns); a sample goes to the first bucket whose
 * bound it is strictly below, otherwise to the last one.  upe_latency_init zeroes everything
 * except min_ns = 1000000, so min_ns never exceeds 1000000 and an empty histogram reports that.
 *
 * One sample (src/latency.c:41-59): ns = (uint64_t)((double)cycles / cycles_per_ns) in exact
 * IEEE-754 double arithmetic — the conversion to double rounds to nearest even, the division is
 * one correctly rounded division, the conversion back truncates — then buckets[b] += 1,
 * total_count += 1, sum_ns += ns (modulo 2^64), min_ns and max_ns updated.
 *
 * Which packets (the batch forms): packet k is sampled iff timestamps[k] > 0 (src/worker.c:120:
 * a buffer nobody stamped is not sampled) and the code of verdicts[k] is not UPE_V_CONSUMED;
 * cycles = now - timestamps[k] as a 64-bit wrapping subtraction.  ARP packets are sampled (they
 * leave through the parse-fail exit whether or not a reply was sent).  verdicts == NULL: nothing
 * was consumed.
 *
 * `now` is ONE value per call: the caller's TSC reading at the point it considers the batch done.
 * A batch finishes as a whole, so this is the batch's completion time, not a per-packet instant;
 * the reference reads the TSC once per packet, at that packet's exit.
 *
 * Where the reference is undefined and this library is not.  The reference divides by a
 * g_cycles_per_ns that defaults to 0.0, and a quotient of 2^64 or more is undefined behaviour in
 * its cast.  Here a calibration that is not finite and > 0 is refused (-1, nothing changes), and
 * ns saturates at UINT64_MAX for a quotient of 2^64 or more.  upe_latency_percentile takes a
 * percentile below 0 (or NaN) as 0 and a target of 2^64 or more as UINT64_MAX.
 *
 * upe_latency_percentile and upe_latency_merge follow src/latency.c:61-90: the upper bound of the
 * first bucket at which the cumulative count reaches (uint64_t)(percentile * total_count), 0 for
 * an empty histogram; counts and sums added, min and max combined.  The stats thread merges the
 * per-worker (here: per-context) histograms this way before printing (src/main.c:317-351).
 *
 * Host functions (upe_host.c; no GPU; messages in upe_host_last_error()).
 * upe_latency_record_batch is upe_gpu_latency_record's exact host equivalent. */
#define UPE_LATENCY_BUCKETS 8
#define UPE_LATENCY_BOUNDS 100, 500, 1000, 5000, 10000, 50000, 100000, 1000000
#define UPE_LATENCY_MIN_INIT 1000000
typedef struct {
    uint64_t buckets[UPE_LATENCY_BUCKETS];
    uint64_t total_count;
    uint64_t min_ns;
    uint64_t max_ns;
    uint64_t sum_ns;
} upe_latency_hist_t;

void upe_latency_init(upe_latency_hist_t *h);
int upe_latency_record(upe_latency_hist_t *h, uint64_t cycles, double cycles_per_ns);
uint64_t upe_latency_percentile(const upe_latency_hist_t *h, double percentile);
void upe_latency_merge(upe_latency_hist_t *dst, const upe_latency_hist_t *src);
int upe_latency_record_batch(upe_latency_hist_t *h, const uint64_t *timestamps,
                             const uint32_t *verdicts, /* optional */
                             size_t n, uint64_t now, double cycles_per_ns);

/* The context's calibration, as worker_set_tsc_calibration (src/worker.c:346) sets the workers' —
 * here per context.  cycles_per_ns must be finite and > 0: -1 otherwise, and the previous value
 * stays.  Measuring it is the caller's business (the caller owns its clock). */
int upe_gpu_set_tsc(upe_gpu_ctx_t *ctx, double cycles_per_ns);

/* Sample a batch on the device into the histogram the context owns there (it accumulates, as the
 * counters do): d_timestamp (device, n uint64 — upe_gpu_ingress_gather's d_timestamp as it
 * stands), d_verdict (device, n uint32 as a classify call left them; NULL = nothing consumed),
 * `now` as above, the calibration last set.  Asynchronous on `stream`; one launch.  The result
 * does not depend on the order in which the device visits the packets (integer adds, min, max).
 * n == 0 launches nothing.  -1 before any launch: a NULL context; NULL timestamps with n > 0; n
 * beyond the kernel's 32-bit indexes; no successful upe_gpu_set_tsc yet.
 * UPE_LATENCY_BLOCK: packets per workgroup pass of the kernel (batch sizes around it are where
 * tests look). */
#define UPE_LATENCY_BLOCK 1024
int upe_gpu_latency_record(upe_gpu_ctx_t *ctx, const uint64_t *d_timestamp,
                           const uint32_t *d_verdict, size_t n, uint64_t now, void *stream);

/* The histogram so far (synchronises), and back to the upe_latency_init state.  Nothing else
 * resets it: upe_gpu_reset_stats, upe_gpu_load_rules, the reloads and upe_gpu_load_neigh leave
 * it alone, as the reference keeps latency_hist across a SIGHUP. */
int upe_gpu_get_latency(upe_gpu_ctx_t *ctx, upe_latency_hist_t *out);
int upe_gpu_reset_latency(upe_gpu_ctx_t *ctx);

/* Kernel timing. enable = k > 0: every k-th upe_gpu_process() call (calls k/2, k/2 + k, ...
 * after enabling: not the first, which starts from an idle queue) records HIP events on its
 * stream around its launches (classify, plus the rule_stats group-by
 * pass of tables over 4096 rules); sampling keeps the events' own queue cost out of a throughput
 * run.  enable = 0 turns timing off.  upe_gpu_timing_span(ctx, every, span): each sample's
 * event pair brackets `span` consecutive calls instead of one, so the events' own latency is
 * spread over `span` launches (the time then includes the gaps between those launches).
 * upe_gpu_timing_read() synchronises and returns the summed time (ms) of the closed samples and
 * the number of calls they cover: classify_ms up to the end of each sample's last classify
 * launch, finalize_ms from there to the end of its rule_stats group-by (0 for tables of up to
 * 4096 rules, which have none). */
int upe_gpu_timing_enable(upe_gpu_ctx_t *ctx, int enable);
int upe_gpu_timing_span(upe_gpu_ctx_t *ctx, int every, int span);
int upe_gpu_timing_read(upe_gpu_ctx_t *ctx, double *classify_ms, double *finalize_ms,
                        uint64_t *launches);

/* Device memory helpers so a C caller needs no HIP headers. */
void *upe_gpu_malloc(upe_gpu_ctx_t *ctx, size_t bytes);
int upe_gpu_free(upe_gpu_ctx_t *ctx, void *dptr);
int upe_gpu_memcpy_h2d(upe_gpu_ctx_t *ctx, void *dst, const void *src, size_t bytes, void *stream);
int upe_gpu_memcpy_d2h(upe_gpu_ctx_t *ctx, void *dst, const void *src, size_t bytes, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Host-side batch builders (upe_amd/csrc/upe_host.c, C)                                      */
/* ------------------------------------------------------------------------------------------ */

/* Load a rule file in the reference's INI format (reference src/rule_config.c:129-282,
 * rules.example) into rules[0..capacity) as rule_table_init(capacity) + rule_config_load would
 * leave rt->rules: rule_id = insertion index, wildcard addresses zeroed, sorted by
 * (priority, rule_id) (src/rule_table.c:130-161).  *count = rules loaded.  0 / -1 (the message,
 * with the reference's "rules:<line>: ..." wording, in upe_host_last_error()). */
int upe_rules_load_ini(const char *path, upe_rule_t *rules, size_t capacity, size_t *count);

/* A pcap capture (LE/BE, usec/nsec, link type Ethernet) -> the packed batch layout above, in
 * record order, as reference src/rx_pcap.c:42-93 admits packets: records with caplen > 2048
 * (PKTBUF_DATA_SIZE) are dropped.  Call with frames = desc = NULL to size the buffers
 * (info->packets descriptors, info->frames_bytes bytes including the UPE_FRAME_TAIL), then again
 * to fill them.  0 / -1. */
typedef struct {
    uint64_t records;          /* records in the file */
    uint64_t packets;          /* packets in the batch */
    uint64_t dropped_oversize; /* caplen > 2048: dropped by RX, never reach the worker */
    uint64_t frames_bytes;     /* frames buffer size needed */
} upe_pcap_info_t;
int upe_pcap_read(const char *path, uint8_t *frames, size_t frames_cap, uint64_t *desc,
                  size_t desc_cap, upe_pcap_info_t *info);

/* Last error of the host-side builders on this thread ("" if none). */
const char *upe_host_last_error(void);

#ifdef __cplusplus
}
#endif

/* Layout checks against the reference (LP64). */
#ifdef __cplusplus
#define UPE_STATIC_ASSERT static_assert
#else
#define UPE_STATIC_ASSERT _Static_assert
#endif
UPE_STATIC_ASSERT(sizeof(upe_gpu_batch_t) == 40, "upe_gpu_batch_t layout");
UPE_STATIC_ASSERT(sizeof(upe_flow_key_t) == 44, "flow_key_t layout");
UPE_STATIC_ASSERT(offsetof(upe_flow_key_t, dst_ip) == 20, "flow_key_t.dst_ip");
UPE_STATIC_ASSERT(offsetof(upe_flow_key_t, protocol) == 40, "flow_key_t.protocol");
UPE_STATIC_ASSERT(sizeof(upe_rule_t) == 92, "rule_t layout");
UPE_STATIC_ASSERT(offsetof(upe_rule_t, src_ip) == 8, "rule_t.src_ip");
UPE_STATIC_ASSERT(offsetof(upe_rule_t, dst_mask) == 56, "rule_t.dst_mask");
UPE_STATIC_ASSERT(offsetof(upe_rule_t, src_port) == 72, "rule_t.src_port");
UPE_STATIC_ASSERT(offsetof(upe_rule_t, protocol) == 76, "rule_t.protocol");
UPE_STATIC_ASSERT(offsetof(upe_rule_t, action) == 80, "rule_t.action");
UPE_STATIC_ASSERT(offsetof(upe_rule_t, rule_id) == 88, "rule_t.rule_id");
UPE_STATIC_ASSERT(sizeof(upe_arp_entry_t) == 32, "arp_entry_t layout");
UPE_STATIC_ASSERT(offsetof(upe_arp_entry_t, valid) == 24, "arp_entry_t.valid");
UPE_STATIC_ASSERT(sizeof(upe_ndp_entry_t) == 40, "ndp_entry_t layout");
UPE_STATIC_ASSERT(offsetof(upe_ndp_entry_t, valid) == 32, "ndp_entry_t.valid");
UPE_STATIC_ASSERT(sizeof(upe_rule_stat_t) == 16, "rule_stat_t layout");
UPE_STATIC_ASSERT(sizeof(upe_hdr_rec_t) == 16, "upe_hdr_rec_t layout");
UPE_STATIC_ASSERT(sizeof(upe_launch_info_t) == 24, "upe_launch_info_t layout");
UPE_STATIC_ASSERT(sizeof(upe_egress_info_t) == 32, "upe_egress_info_t layout");
UPE_STATIC_ASSERT(sizeof(upe_pktbuf_t) == 2064, "pktbuf_t layout");
UPE_STATIC_ASSERT(offsetof(upe_pktbuf_t, len) == 8, "pktbuf_t.len");
UPE_STATIC_ASSERT(offsetof(upe_pktbuf_t, data) == 16, "pktbuf_t.data");
UPE_STATIC_ASSERT(sizeof(upe_ingress_info_t) == 64, "upe_ingress_info_t layout");
UPE_STATIC_ASSERT(sizeof(upe_ctrl_write_t) == 32, "upe_ctrl_write_t layout");
UPE_STATIC_ASSERT(offsetof(upe_ctrl_write_t, mac_off) == 6, "upe_ctrl_write_t.mac_off");
UPE_STATIC_ASSERT(offsetof(upe_ctrl_write_t, mac) == 8, "upe_ctrl_write_t.mac");
UPE_STATIC_ASSERT(offsetof(upe_ctrl_write_t, ip) == 16, "upe_ctrl_write_t.ip");
UPE_STATIC_ASSERT(sizeof(upe_ctrl_info_t) == 32, "upe_ctrl_info_t layout");
UPE_STATIC_ASSERT(sizeof(upe_neigh_learn_info_t) == 64, "upe_neigh_learn_info_t layout");
UPE_STATIC_ASSERT(sizeof(upe_neigh_image_info_t) == 32, "upe_neigh_image_info_t layout");
UPE_STATIC_ASSERT(sizeof(upe_release_info_t) == 64, "upe_release_info_t layout");
UPE_STATIC_ASSERT(sizeof(upe_latency_hist_t) == 96, "latency_histogram_t layout");
UPE_STATIC_ASSERT(offsetof(upe_latency_hist_t, total_count) == 64, "latency_histogram_t.total_count");
UPE_STATIC_ASSERT(offsetof(upe_latency_hist_t, min_ns) == 72, "latency_histogram_t.min_ns");
UPE_STATIC_ASSERT(offsetof(upe_latency_hist_t, max_ns) == 80, "latency_histogram_t.max_ns");
UPE_STATIC_ASSERT(offsetof(upe_latency_hist_t, sum_ns) == 88, "latency_histogram_t.sum_ns");

#endif /* UPE_GPU_H */
