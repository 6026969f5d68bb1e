/*
 * upe_host.c — host-side batch builders around the MI355X path (C, linked into libupe_gpu.so).
 *
 * These are the two rows SURVEY.md §8(f) ranks next to the kernel: the rule-file loader that
 * fills the table the kernel classifies against, and the ingress batch builder that turns a
 * capture into the packed batch layout of include/upe_gpu.h.  Both restate the reference's
 * behaviour from its sources (no reference code is compiled in):
 *
 *   upe_rules_load_ini  reference src/rule_config.c:129-282 (rule_config_load) into a table of
 *                       rule_table_init(capacity) with rule_table_add semantics
 *                       (src/rule_table.c:130-161): rule_id = insertion index, wildcard addresses
 *                       zeroed, sorted by (priority, rule_id).
 *   upe_pcap_read       the capture side of reference src/rx_pcap.c:42-93 / 95-167 for a pcap
 *                       file: every record in file order, caplen > PKTBUF_DATA_SIZE (2048)
 *                       dropped (src/rx_pcap.c:53-57), the rest packed at 16-byte aligned offsets.
 *   upe_hdr_apply       an emit-mode record (upe_hdr_rec_t) applied to its frame: the rewrite of
 *                       src/worker.c:162-244 as bytes.
 *   upe_latency_*       the worker's latency histogram (reference include/latency.h:21-40,
 *                       src/latency.c:35-90) and the host equivalent of upe_gpu_latency_record.
 *   upe_neigh_lookup_host  arp_get_mac / ndp_get_mac (src/arp_table.c:55-80,
 *                       src/ndp_table.c:67-86) per flow key over the slot arrays: the host
 *                       equivalent of upe_gpu_resolve_keys.
 *   upe_ctrl_writes_host   the table writes of handle_control_packet (src/worker.c:23-104) for a
 *                       batch, as records: the host equivalent of upe_gpu_ctrl_writes.
 *   upe_neigh_apply_writes arp_update / ndp_update (src/arp_table.c:26-53,
 *                       src/ndp_table.c:39-65) of those records on the slot arrays.
 *   upe_release_order_host the order in which worker_main frees a classified batch's buffers
 *                       (src/worker.c:280-303): the host equivalent of upe_gpu_release_order.
 *   upe_release_flush   worker_main's tx_send, tx_send_batch and pktbuf_free calls from those lists.
 */
#define _GNU_SOURCE
#include <arpa/inet.h>
#include <ctype.h>
#include <errno.h>
#include <float.h>
#include <net/if.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/upe_gpu.h"

static __thread char g_host_err[256];

static int host_fail(const char *fmt, int line, const char *what) {
    snprintf(g_host_err, sizeof g_host_err, fmt, line, what ? what : "");
    return -1;
}

const char *upe_host_last_error(void) { return g_host_err; }

/* ---- rule file (INI) -------------------------------------------------------------------- */

#define UPE_MAX_LINE 512 /* src/rule_config.c:18: longer lines are read in pieces, as fgets does */

static char *strip(char *s) { /* src/rule_config.c:20-32 */
    while (*s && isspace((unsigned char)*s)) s++;
    char *end = s + strlen(s);
    while (end > s && isspace((unsigned char)end[-1])) end--;
    *end = '\0';
    return s;
}

static int mask4(uint8_t prefix, uint32_t *out) { /* src/rule_table.c:14-30 */
    if (prefix > 32) return 0;
    *out = prefix == 0 ? 0u : (uint32_t)(0xFFFFFFFFu << (32 - prefix));
    return 1;
}

static int mask6(uint8_t prefix, uint8_t out[16]) { /* src/rule_table.c:32-50 */
    if (prefix > 128) return 0;
    for (int i = 0; i < 16; i++) {
        int bits = (int)prefix - 8 * i;
        out[i] = bits >= 8 ? 0xFF : bits <= 0 ? 0 : (uint8_t)(0xFF << (8 - bits));
    }
    return 1;
}

/* "addr[/prefix]" -> address + mask, src/rule_config.c:38-91 (the prefix is taken modulo 256,
 * as the reference's uint8_t cast does; no prefix means a host route). */
static int parse_ip_prefix(const char *str, uint8_t *ver, upe_ip_addr_t *ip, upe_ip_addr_t *mask) {
    char buf[INET6_ADDRSTRLEN + 4];
    strncpy(buf, str, sizeof buf - 1);
    buf[sizeof buf - 1] = '\0';
    char *slash = strchr(buf, '/');
    uint8_t plen = 255;
    if (slash) {
        *slash = '\0';
        errno = 0;
        char *end = NULL;
        long pl = strtol(slash + 1, &end, 10);
        if (errno != 0 || end == slash + 1 || *end != '\0' || pl < 0) return -1;
        plen = (uint8_t)pl;
    }
    memset(ip, 0, sizeof *ip);
    memset(mask, 0, sizeof *mask);
    struct in_addr a4;
    if (inet_pton(AF_INET, buf, &a4) == 1) {
        *ver = 4;
        ip->v4 = ntohl(a4.s_addr);
        return mask4(plen == 255 ? 32 : plen, &mask->v4) ? 0 : -1;
    }
    struct in6_addr a6;
    if (inet_pton(AF_INET6, buf, &a6) == 1) {
        *ver = 6;
        memcpy(ip->v6, a6.s6_addr, 16);
        return mask6(plen == 255 ? 128 : plen, mask->v6) ? 0 : -1;
    }
    return -1;
}

static uint8_t parse_protocol(const char *v) { /* src/rule_config.c:93-106 */
    if (strcmp(v, "tcp") == 0) return 6;
    if (strcmp(v, "udp") == 0) return 17;
    if (strcmp(v, "icmp") == 0) return 1;
    if (strcmp(v, "icmpv6") == 0) return 58;
    errno = 0;
    char *end = NULL;
    long x = strtol(v, &end, 10);
    if (errno == 0 && end != v && *end == '\0' && x >= 0 && x <= 255) return (uint8_t)x;
    return 0;
}

static int parse_long(const char *v, long lo, long hi, long *out) {
    errno = 0;
    char *end = NULL;
    long x = strtol(v, &end, 10);
    if (errno != 0 || end == v || *end != '\0' || x < lo || x > hi) return -1;
    *out = x;
    return 0;
}

/* rule_table_add, src/rule_table.c:130-161 (the sort happens once, at the end: the comparator
 * is a total order over unique rule_ids, so the result is the same). */
static int table_add(upe_rule_t *rules, size_t capacity, size_t *count, const upe_rule_t *in) {
    if (*count >= capacity) return -1;
    upe_rule_t r = *in;
    r.rule_id = (uint32_t)*count;
    static const uint8_t zero16[16];
    if (r.ip_ver == 4 && r.src_mask.v4 == 0) r.src_ip.v4 = 0;
    if (r.ip_ver == 4 && r.dst_mask.v4 == 0) r.dst_ip.v4 = 0;
    if (r.ip_ver == 6) {
        if (memcmp(r.src_mask.v6, zero16, 16) == 0) memset(r.src_ip.v6, 0, 16);
        if (memcmp(r.dst_mask.v6, zero16, 16) == 0) memset(r.dst_ip.v6, 0, 16);
    }
    rules[(*count)++] = r;
    return 0;
}

static int rule_cmp(const void *a, const void *b) { /* src/rule_table.c:96-109 */
    const upe_rule_t *x = a, *y = b;
    if (x->priority != y->priority) return x->priority < y->priority ? -1 : 1;
    if (x->rule_id != y->rule_id) return x->rule_id < y->rule_id ? -1 : 1;
    return 0;
}

static int flush_rule(upe_rule_t *r, int *active, upe_rule_t *rules, size_t capacity,
                      size_t *count, int line) { /* src/rule_config.c:112-127 */
    if (!*active) return 0;
    *active = 0;
    if (r->action.type == UPE_ACT_FWD && r->action.out_ifindex == 0)
        return host_fail("rules:%d: fwd rule missing out_iface%s", line, "");
    if (table_add(rules, capacity, count, r) != 0)
        return host_fail("rules:%d: failed to add rule (table may be full)%s", line, "");
    return 0;
}

int upe_rules_load_ini(const char *path, upe_rule_t *rules, size_t capacity, size_t *count) {
    if (!path || !rules || !count || capacity == 0) return host_fail("rules:%d: bad argument%s", 0, "");
    FILE *f = fopen(path, "r");
    if (!f) return host_fail("rules:%d: unable to open %s", 0, path);
    *count = 0;
    char line[UPE_MAX_LINE];
    int ln = 0, active = 0, rc = 0;
    upe_rule_t cur;
    memset(&cur, 0, sizeof cur);
    while (rc == 0 && fgets(line, UPE_MAX_LINE, f)) {
        ln++;
        line[strcspn(line, "\r\n")] = '\0';
        char *s = strip(line);
        if (*s == '\0' || *s == '#' || *s == ';') continue;
        if (*s == '[') {
            if ((rc = flush_rule(&cur, &active, rules, capacity, count, ln)) != 0) break;
            if (strncmp(s, "[rule]", 6) != 0) {
                rc = host_fail("rules:%d: unknown section header: %s", ln, s);
                break;
            }
            memset(&cur, 0, sizeof cur);
            active = 1;
            continue;
        }
        if (!active) {
            rc = host_fail("rules:%d: key=value outside [rule] section%s", ln, "");
            break;
        }
        char *eq = strchr(s, '=');
        if (!eq) {
            rc = host_fail("rules:%d: expected key = value%s", ln, "");
            break;
        }
        *eq = '\0';
        char *key = strip(s), *val = strip(eq + 1);
        long x;
        uint8_t ver = 0;
        if (strcmp(key, "priority") == 0) {
            if (parse_long(val, 0, __LONG_MAX__, &x) != 0) rc = host_fail("rules:%d: invalid priority: %s", ln, val);
            else cur.priority = (uint32_t)x;
        } else if (strcmp(key, "ip_version") == 0) {
            if (strcmp(val, "4") == 0) cur.ip_ver = 4;
            else if (strcmp(val, "6") == 0) cur.ip_ver = 6;
            else rc = host_fail("rules:%d: invalid ip_version: %s", ln, val);
        } else if (strcmp(key, "protocol") == 0) {
            cur.protocol = parse_protocol(val);
        } else if (strcmp(key, "src") == 0 || strcmp(key, "dst") == 0) {
            const int src = key[0] == 's';
            if (parse_ip_prefix(val, &ver, src ? &cur.src_ip : &cur.dst_ip,
                                src ? &cur.src_mask : &cur.dst_mask) != 0)
                rc = host_fail(src ? "rules:%d: invalid src address: %s"
                                   : "rules:%d: invalid dst address: %s", ln, val);
            else if (cur.ip_ver == 0)
                cur.ip_ver = ver;
        } else if (strcmp(key, "src_port") == 0 || strcmp(key, "dst_port") == 0) {
            if (parse_long(val, 0, 65535, &x) != 0)
                rc = host_fail("rules:%d: invalid port: %s", ln, val);
            else if (key[0] == 's')
                cur.src_port = (uint16_t)x;
            else
                cur.dst_port = (uint16_t)x;
        } else if (strcmp(key, "action") == 0) {
            if (strcmp(val, "drop") == 0) cur.action.type = UPE_ACT_DROP;
            else if (strcmp(val, "fwd") == 0) cur.action.type = UPE_ACT_FWD;
            else rc = host_fail("rules:%d: invalid action: %s", ln, val);
        } else if (strcmp(key, "out_iface") == 0) {
            unsigned idx = if_nametoindex(val);
            if (idx == 0) rc = host_fail("rules:%d: unknown interface: %s", ln, val);
            else cur.action.out_ifindex = (int32_t)idx;
        } else {
            rc = host_fail("rules:%d: unknown key: %s", ln, key);
        }
    }
    if (rc == 0) rc = flush_rule(&cur, &active, rules, capacity, count, ln);
    fclose(f);
    if (rc != 0) return -1;
    qsort(rules, *count, sizeof(upe_rule_t), rule_cmp);
    return 0;
}

/* ---- pcap capture -> packed batch --------------------------------------------------------- */

#define PKTBUF_DATA_SIZE 2048 /* reference include/pktbuf.h:8 */

static uint32_t rd32(const uint8_t *p, int swap) {
    uint32_t v;
    memcpy(&v, p, 4);
    return swap ? __builtin_bswap32(v) : v;
}

int upe_pcap_read(const char *path, uint8_t *frames, size_t frames_cap, uint64_t *desc,
                  size_t desc_cap, upe_pcap_info_t *info) {
    if (!path || !info) return host_fail("pcap:%d: bad argument%s", 0, "");
    memset(info, 0, sizeof *info);
    FILE *f = fopen(path, "rb");
    if (!f) return host_fail("pcap:%d: unable to open %s", 0, path);
    uint8_t gh[24];
    if (fread(gh, 1, 24, f) != 24) {
        fclose(f);
        return host_fail("pcap:%d: short global header%s", 0, "");
    }
    uint32_t magic;
    memcpy(&magic, gh, 4);
    int swap;
    if (magic == 0xa1b2c3d4u || magic == 0xa1b23c4du) swap = 0;
    else if (magic == 0xd4c3b2a1u || magic == 0x4d3cb2a1u) swap = 1;
    else {
        fclose(f);
        return host_fail("pcap:%d: not a pcap file (magic)%s", 0, "");
    }
    if (rd32(gh + 20, swap) != 1) {
        fclose(f);
        return host_fail("pcap:%d: link type is not Ethernet%s", 0, "");
    }
    const int fill = frames && desc;
    size_t cursor = 0, n = 0;
    uint8_t rh[16];
    uint8_t *buf = malloc(65536 * 4);
    if (!buf) {
        fclose(f);
        return host_fail("pcap:%d: out of memory%s", 0, "");
    }
    int rc = 0;
    for (;;) {
        size_t got = fread(rh, 1, 16, f);
        if (got == 0) break;
        if (got != 16) {
            rc = host_fail("pcap:%d: truncated record header%s", (int)info->records, "");
            break;
        }
        const uint32_t caplen = rd32(rh + 8, swap);
        if (caplen > 65536u * 4) {
            rc = host_fail("pcap:%d: record too large%s", (int)info->records, "");
            break;
        }
        if (fread(buf, 1, caplen, f) != caplen) {
            rc = host_fail("pcap:%d: truncated record%s", (int)info->records, "");
            break;
        }
        info->records++;
        if (caplen > PKTBUF_DATA_SIZE) { /* src/rx_pcap.c:53-57 */
            info->dropped_oversize++;
            continue;
        }
        const size_t sz = caplen ? (caplen + 15u) & ~(size_t)15u : 16u;
        if (fill) {
            if (n >= desc_cap || cursor + sz + UPE_FRAME_TAIL > frames_cap) {
                rc = host_fail("pcap:%d: batch buffers too small%s", (int)info->records, "");
                break;
            }
            memcpy(frames + cursor, buf, caplen);
            memset(frames + cursor + caplen, 0, sz - caplen);
            desc[n] = UPE_DESC(cursor, caplen);
        }
        cursor += sz;
        n++;
    }
    free(buf);
    fclose(f);
    info->packets = n;
    info->frames_bytes = cursor + UPE_FRAME_TAIL;
    if (rc == 0 && fill) memset(frames + cursor, 0, UPE_FRAME_TAIL);
    return rc;
}

/* ---- emit-mode records ------------------------------------------------------------------- */

/* The bytes process_packet leaves in a forwarded frame (reference src/worker.c:174-176 TTL and
 * checksum, :197-200 / :227-230 MACs, :213 hop limit), from a upe_hdr_rec_t. */
void upe_hdr_apply(uint8_t *frame, const upe_hdr_rec_t *rec) {
    const uint8_t fam = rec->b[15];
    if (fam != 4 && fam != 6) return;
    memcpy(frame, rec->b, 12);
    if (fam == 4) {
        frame[22] = rec->b[12];
        frame[24] = rec->b[13];
        frame[25] = rec->b[14];
    } else {
        frame[21] = rec->b[12];
    }
}

/* ---- egress ------------------------------------------------------------------------------ */

/* The TX side of the worker loop (src/worker.c:240-243 queue, :287-303 flush): per input burst,
 * the forwarded frames in packet order go to one tx_send_batch-like call. */
int upe_tx_flush(const uint8_t *h_frames, const uint64_t *h_desc, const uint32_t *h_verdict,
                 size_t n, size_t burst, upe_tx_batch_fn send, void *user, uint64_t *forwarded,
                 uint64_t *dropped) {
    if (burst == 0 || burst > UPE_TX_BATCH_MAX)
        return host_fail("upe_tx_flush: burst %d must be 1..UPE_TX_BATCH_MAX", (int)burst, "");
    if (n && (!h_frames || !h_desc || !h_verdict || !send))
        return host_fail("upe_tx_flush: null argument%.0d%s", 0, "");
    const uint8_t *frames[UPE_TX_BATCH_MAX];
    size_t lens[UPE_TX_BATCH_MAX];
    for (size_t base = 0; base < n; base += burst) {
        const size_t end = n - base < burst ? n : base + burst;
        int count = 0;
        for (size_t i = base; i < end; i++) {
            if (UPE_VERDICT_CODE(h_verdict[i]) != UPE_V_FWD) continue;
            frames[count] = h_frames + (h_desc[i] >> 16);
            lens[count++] = (size_t)(h_desc[i] & 0xFFFFu);
        }
        if (count == 0) continue;   /* src/worker.c:287: no call for an all-dropped burst */
        int sent = send(user, frames, lens, count);
        if (sent < 0) sent = 0;
        if (sent > count) sent = count;
        if (forwarded) *forwarded += (uint64_t)sent;
        if (dropped) *dropped += (uint64_t)(count - sent);
    }
    return 0;
}

int upe_tx_flush_groups(const uint8_t *h_frames, const uint64_t *h_desc, const uint32_t *h_tx,
                        const uint32_t *h_tx_count, size_t n, size_t burst, upe_tx_batch_fn send,
                        void *user, uint64_t *forwarded, uint64_t *dropped) {
    if (burst == 0 || burst > UPE_TX_BATCH_MAX)
        return host_fail("upe_tx_flush_groups: burst %d must be 1..UPE_TX_BATCH_MAX", (int)burst, "");
    if (n && (!h_frames || !h_desc || !h_tx || !h_tx_count || !send))
        return host_fail("upe_tx_flush_groups: null argument%.0d%s", 0, "");
    const uint8_t *frames[UPE_TX_BATCH_MAX];
    size_t lens[UPE_TX_BATCH_MAX];
    size_t g = 0, k = 0; /* the next list entry: group g, its k-th forwarded packet */
    for (size_t base = 0; base < n; base += burst) {
        const size_t end = n - base < burst ? n : base + burst;
        int count = 0;
        for (;;) {
            if (g * 64 >= end || g * 64 >= n) break;
            const uint32_t cnt = h_tx_count[g];
            if (cnt > 64) return host_fail("upe_tx_flush_groups: group count %d above 64", (int)cnt, "");
            if (k >= cnt) { g++; k = 0; continue; }
            const uint32_t i = h_tx[g * 64 + k];
            if (i >= end) break; /* the next burst's */
            if (i < base || count == (int)burst)
                return host_fail("upe_tx_flush_groups: list entry %d out of packet order%s", (int)i, "");
            frames[count] = h_frames + (h_desc[i] >> 16);
            lens[count++] = (size_t)(h_desc[i] & 0xFFFFu);
            k++;
        }
        if (count == 0) continue; /* src/worker.c:287: no call for an all-dropped burst */
        int sent = send(user, frames, lens, count);
        if (sent < 0) sent = 0;
        if (sent > count) sent = count;
        if (forwarded) *forwarded += (uint64_t)sent;
        if (dropped) *dropped += (uint64_t)(count - sent);
    }
    return 0;
}

/* The same calls from the packed egress batch of upe_gpu_egress_pack: frame k lies at
 * h_out + (h_out_desc[k] >> 16) and belongs to input burst h_out_index[k] / burst.  Everything is
 * checked before the first send (all or nothing). */
int upe_tx_flush_packed(const uint8_t *h_out, const uint64_t *h_out_desc,
                        const uint32_t *h_out_index, size_t count, size_t burst,
                        upe_tx_batch_fn send, void *user, uint64_t *forwarded, uint64_t *dropped) {
    if (burst == 0 || burst > UPE_TX_BATCH_MAX)
        return host_fail("upe_tx_flush_packed: burst %d must be 1..UPE_TX_BATCH_MAX", (int)burst, "");
    if (count && (!h_out || !h_out_desc || !h_out_index || !send))
        return host_fail("upe_tx_flush_packed: null argument%.0d%s", 0, "");
    for (size_t k = 1; k < count; k++)
        if (h_out_index[k] <= h_out_index[k - 1])
            return host_fail("upe_tx_flush_packed: index list entry %d does not ascend%s", (int)k, "");
    const uint8_t *frames[UPE_TX_BATCH_MAX];
    size_t lens[UPE_TX_BATCH_MAX];
    size_t k = 0;
    while (k < count) {
        /* strictly ascending indexes: a burst holds at most `burst` <= UPE_TX_BATCH_MAX of them */
        const size_t b = h_out_index[k] / burst;
        int c = 0;
        for (; k < count && h_out_index[k] / burst == b; k++) {
            frames[c] = h_out + (h_out_desc[k] >> 16);
            lens[c++] = (size_t)(h_out_desc[k] & 0xFFFFu);
        }
        int sent = send(user, frames, lens, c);
        if (sent < 0) sent = 0;
        if (sent > c) sent = c;
        if (forwarded) *forwarded += (uint64_t)sent;
        if (dropped) *dropped += (uint64_t)(c - sent);
    }
    return 0;
}

/* ---- release order ----------------------------------------------------------------------- */

/* The burst description both release functions take: -1 for one that no call accepts. */
static int release_bursts_ok(const char *who, const uint32_t *first, size_t nb, uint32_t burst,
                             size_t n) {
    if (!first && (burst == 0 || burst > UPE_TX_BATCH_MAX))
        return host_fail("%.0d%s: burst must be 1..UPE_TX_BATCH_MAX", 0, who);
    if (first && ((nb == 0 && n > 0) || nb > n))
        return host_fail("%.0d%s: an offset array describes 1..n bursts", 0, who);
    if (n > 0xFFFFFFFFull - UPE_RELEASE_BLOCK)
        return host_fail("%.0d%s: n must fit in 32 bits", 0, who);
    return 0;
}

/* The violated conditions of an offset array (upe_release_info_t.bad_bursts). */
static uint64_t release_bad_bursts(const uint32_t *first, size_t nb, size_t n) {
    uint64_t bad = (first[0] != 0u) + (first[nb] != (uint32_t)n);
    for (size_t b = 0; b < nb; b++)
        if ((uint32_t)(first[b + 1] - first[b] - 1u) >= UPE_TX_BATCH_MAX) bad++;
    return bad;
}

/* Burst b of n packets: [*s, *e). */
static void release_burst(const uint32_t *first, uint32_t burst, size_t n, size_t b, size_t *s,
                          size_t *e) {
    if (first) {
        *s = first[b];
        *e = first[b + 1];
    } else {
        *s = b * burst;
        *e = n - *s < burst ? n : *s + burst;
    }
}

/* The frees of worker_main in their order (src/worker.c:280-303): per burst the buffers
 * process_packet frees at its exits, then tx_bufs[]. */
int upe_release_order_host(const uint32_t *verdict, size_t n, const uint32_t *burst_first,
                           size_t nb, uint32_t burst, const uint32_t *slot, uint32_t *order,
                           uint32_t *handle, uint32_t *burst_fwd, uint32_t *reply,
                           upe_release_info_t *info) {
    if (!info || (n && (!verdict || !order || !burst_fwd)))
        return host_fail("upe_release_order_host: null argument%.0d%s", 0, "");
    if ((slot == NULL) != (handle == NULL))
        return host_fail("upe_release_order_host: slot and handle go together%.0d%s", 0, "");
    if (release_bursts_ok("upe_release_order_host", burst_first, nb, burst, n) != 0) return -1;
    upe_release_info_t x;
    memset(&x, 0, sizeof x);
    x.packets = n;
    x.first_reply = UINT64_MAX;
    for (size_t i = 0; i < n; i++) {
        const uint32_t code = UPE_VERDICT_CODE(verdict[i]);
        if (code == UPE_V_FWD) x.forwarded++;
        else if (code == UPE_V_CONSUMED) x.consumed++;
        else x.dropped++;
        if (verdict[i] & UPE_VF_ARP_REPLY) {
            if (x.replies++ == 0) x.first_reply = i;
        }
    }
    if (n == 0) {
        *info = x;
        return 0;
    }
    x.bursts = burst_first ? nb : (n + burst - 1) / burst;
    if (burst_first) x.bad_bursts = release_bad_bursts(burst_first, nb, n);
    *info = x;
    if (x.bad_bursts) return 0;   /* reported in *info; no other output is touched */
    for (size_t b = 0; b < x.bursts; b++) {
        size_t s, e;
        release_burst(burst_first, burst, n, b, &s, &e);
        size_t k = s;
        for (size_t i = s; i < e; i++)
            if (UPE_VERDICT_CODE(verdict[i]) != UPE_V_FWD) order[k++] = (uint32_t)i;
        burst_fwd[b] = (uint32_t)(e - k);
        for (size_t i = s; i < e; i++)
            if (UPE_VERDICT_CODE(verdict[i]) == UPE_V_FWD) order[k++] = (uint32_t)i;
    }
    if (slot)
        for (size_t k = 0; k < n; k++) handle[k] = slot[order[k]];
    if (reply) {
        size_t k = 0;
        for (size_t i = 0; i < n; i++)
            if (verdict[i] & UPE_VF_ARP_REPLY) reply[k++] = (uint32_t)i;
    }
    return 0;
}

/* worker_main's calls from the lists (src/worker.c:51 tx_send, :287-303 the flush and its frees),
 * everything checked before the first one. */
int upe_release_flush(const uint8_t *h_frames, const uint64_t *h_desc, const uint32_t *h_order,
                      const uint32_t *h_handle, const uint32_t *h_burst_first, size_t nb,
                      uint32_t burst, size_t n, const uint32_t *h_burst_fwd,
                      const uint32_t *h_reply, size_t replies, const upe_release_ops_t *ops,
                      void *user, uint64_t *forwarded, uint64_t *dropped) {
    if (release_bursts_ok("upe_release_flush", h_burst_first, nb, burst, n) != 0) return -1;
    if (n && (!h_frames || !h_desc || !h_order || !h_burst_fwd || !ops || !ops->send ||
              !ops->release))
        return host_fail("upe_release_flush: null argument%.0d%s", 0, "");
    if (replies && (!h_reply || !ops || !ops->send_one))
        return host_fail("upe_release_flush: replies without a list or send_one%.0d%s", 0, "");
    if (n && h_burst_first && release_bad_bursts(h_burst_first, nb, n) != 0)
        return host_fail("upe_release_flush: the offset array is not valid%.0d%s", 0, "");
    for (size_t k = 0; k < replies; k++)
        if (h_reply[k] >= n || (k && h_reply[k] <= h_reply[k - 1]))
            return host_fail("upe_release_flush: reply list entry %d is out of order or range%s",
                             (int)k, "");
    const size_t bursts = n == 0 ? 0 : h_burst_first ? nb : (n + burst - 1) / burst;
    for (size_t b = 0; b < bursts; b++) {
        size_t s, e;
        release_burst(h_burst_first, burst, n, b, &s, &e);
        if (h_burst_fwd[b] > e - s)
            return host_fail("upe_release_flush: burst %d forwards more than it holds%s", (int)b, "");
        for (size_t k = s; k < e; k++)
            if (h_order[k] < s || h_order[k] >= e)
                return host_fail("upe_release_flush: order entry %d lies outside its burst%s",
                                 (int)k, "");
    }
    const uint32_t *handles = h_handle ? h_handle : h_order;
    const uint8_t *frames[UPE_TX_BATCH_MAX];
    size_t lens[UPE_TX_BATCH_MAX];
    size_t q = 0; /* the next reply */
    for (size_t b = 0; b < bursts; b++) {
        size_t s, e;
        release_burst(h_burst_first, burst, n, b, &s, &e);
        const size_t f = h_burst_fwd[b], r = e - s - f;
        for (; q < replies && h_reply[q] < e; q++) { /* ascending and < n: inside [s, e) */
            const uint64_t d = h_desc[h_reply[q]];
            ops->send_one(user, h_frames + (d >> 16), (size_t)(d & 0xFFFFu));
        }
        if (r) ops->release(user, handles + s, r);
        if (f == 0) continue; /* src/worker.c:287: no call for a burst that forwarded nothing */
        for (size_t k = 0; k < f; k++) {
            const uint64_t d = h_desc[h_order[s + r + k]];
            frames[k] = h_frames + (d >> 16);
            lens[k] = (size_t)(d & 0xFFFFu);
        }
        int sent = ops->send(user, frames, lens, (int)f);
        if (sent < 0) sent = 0;
        if (sent > (int)f) sent = (int)f;
        if (forwarded) *forwarded += (uint64_t)sent;
        if (dropped) *dropped += (uint64_t)((int)f - sent);
        ops->release(user, handles + s + r, f);
    }
    return 0;
}

int upe_gpu_hdr_layout(void) { return UPE_HDR_LAYOUT; }

/* ---- neighbour lookup ------------------------------------------------------------------- */

static uint32_t ld_le32(const uint8_t *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

/* a hit's MAC in upe_gpu_resolve_keys' format */
static uint64_t mac_found(const uint8_t mac[6]) {
    uint64_t v = UPE_MAC_FOUND;
    for (int j = 0; j < 6; j++) v |= (uint64_t)mac[j] << (8 * j);
    return v;
}

/* src/arp_table.c:55-80: from the address's low bits, the first valid entry of the address;
 * nothing past the first invalid slot */
static uint64_t arp_probe(const upe_arp_entry_t *t, size_t cap, uint32_t ip) {
    for (size_t i = 0, s = ip & (cap - 1); i < cap; i++, s = (s + 1) & (cap - 1)) {
        if (!t[s].valid) break;
        if (t[s].ip == ip) return mac_found(t[s].mac);
    }
    return 0;
}

/* src/ndp_table.c:67-86, from hash_ipv6 (:6-17): the XOR of the four words as the bytes lie */
static uint64_t ndp_probe(const upe_ndp_entry_t *t, size_t cap, const uint8_t ip[16]) {
    const size_t home = ld_le32(ip) ^ ld_le32(ip + 4) ^ ld_le32(ip + 8) ^ ld_le32(ip + 12);
    for (size_t i = 0, s = home & (cap - 1); i < cap; i++, s = (s + 1) & (cap - 1)) {
        if (!t[s].valid) break;
        if (memcmp(t[s].ip, ip, 16) == 0) return mac_found(t[s].mac);
    }
    return 0;
}

int upe_neigh_lookup_host(const upe_arp_entry_t *arp, size_t arp_capacity,
                          const upe_ndp_entry_t *ndp, size_t ndp_capacity,
                          const upe_flow_key_t *keys, size_t n, uint64_t *mac) {
    if ((arp_capacity & (arp_capacity - 1)) != 0 || (ndp_capacity & (ndp_capacity - 1)) != 0)
        return host_fail("upe_neigh_lookup_host: capacity must be a power of two%.0d%s", 0, "");
    if ((arp_capacity && !arp) || (ndp_capacity && !ndp) || (n && (!keys || !mac)))
        return host_fail("upe_neigh_lookup_host: null argument%.0d%s", 0, "");
    for (size_t k = 0; k < n; k++) {
        const uint8_t *d = keys[k].dst_ip.v6;
        mac[k] = keys[k].ip_ver == 4 ? arp_probe(arp, arp_capacity, ld_le32(d))
               : keys[k].ip_ver == 6 ? ndp_probe(ndp, ndp_capacity, d)
                                     : 0;
    }
    return 0;
}

/* ---- control writes --------------------------------------------------------------------- */

/* frame byte j, zero at or past len (a zero-filled pktbuf) */
static uint32_t byte_at(const uint8_t *f, uint32_t len, uint32_t j) { return j < len ? f[j] : 0u; }

/* ctrl_table_write (csrc/upe_dev.h), the rule of upe_gpu_ingress_gather's d_ctrl */
static int ctrl_marked(const uint8_t *f, uint32_t len) {
    const uint32_t et = byte_at(f, len, 12) << 8 | byte_at(f, len, 13);
    if (et == 0x0806u)
        return byte_at(f, len, 14) == 0 && byte_at(f, len, 15) == 1 && byte_at(f, len, 16) == 8 &&
               byte_at(f, len, 17) == 0 && byte_at(f, len, 18) == 6 && byte_at(f, len, 19) == 4;
    return et == 0x86DDu && len >= 78 && byte_at(f, len, 20) == 58 &&
           (byte_at(f, len, 54) == 135 || byte_at(f, len, 54) == 136);
}

/* One marked frame's record (src/worker.c:28-39 ARP, :57-95 NS / NA): 1 when it has one. */
static int ctrl_record(const uint8_t *f, uint32_t len, uint32_t index, upe_ctrl_write_t *w) {
    memset(w, 0, sizeof *w);
    w->index = index;
    if (byte_at(f, len, 12) == 0x08) {
        w->kind = UPE_CW_ARP;
        w->mac_off = 22;
        for (uint32_t j = 0; j < 6; j++) w->mac[j] = (uint8_t)byte_at(f, len, 22 + j);
        /* ntohl(spa) as upe_ip_addr_t.v4 holds it on a little-endian host */
        for (uint32_t j = 0; j < 4; j++) w->ip[j] = (uint8_t)byte_at(f, len, 31 - j);
        return 1;
    }
    const int na = f[54] == 136; /* len >= 78 */
    for (uint32_t off = 78; off + 2 <= len;) {
        const uint8_t ot = f[off];
        const uint8_t ol = (uint8_t)(f[off + 1] * 8u); /* src/worker.c:73: 32 wraps to 0 */
        if (ol == 0 || off + ol > len) break;
        if (ot == (na ? 2 : 1)) {
            w->kind = UPE_CW_NDP;
            w->mac_off = (uint16_t)(off + 2);
            memcpy(w->mac, f + off + 2, 6);
            memcpy(w->ip, f + (na ? 62 : 22), 16);
            return 1;
        }
        off += ol;
    }
    return 0;
}

int upe_ctrl_writes_host(const uint8_t *frames, const uint64_t *desc, size_t n,
                         upe_ctrl_write_t *writes, size_t cap, upe_ctrl_info_t *info) {
    if (!info || (n && (!frames || !desc)) || (cap && !writes))
        return host_fail("upe_ctrl_writes_host: null argument%.0d%s", 0, "");
    if (n > 0xFFFFFFFFull - UPE_CTRL_BLOCK)
        return host_fail("upe_ctrl_writes_host: n must fit in 32 bits%.0d%s", 0, "");
    memset(info, 0, sizeof *info);
    info->first_write = UINT64_MAX;
    for (size_t i = 0; i < n; i++) {
        const uint32_t len = (uint32_t)(desc[i] & 0xFFFFu);
        const uint8_t *f = frames + (desc[i] >> 16);
        if (!ctrl_marked(f, len)) continue;
        info->ctrl++;
        upe_ctrl_write_t w;
        if (!ctrl_record(f, len, (uint32_t)i, &w)) continue;
        if (info->writes == 0) info->first_write = i;
        if (info->writes < cap) writes[info->stored++] = w;
        info->writes++;
    }
    return 0;
}

/* arp_update, src/arp_table.c:26-53: the slot to write, or NULL when the table is full of other
 * addresses. */
static upe_arp_entry_t *arp_slot(upe_arp_entry_t *t, size_t cap, uint32_t ip) {
    for (size_t k = 0, s = ip & (cap - 1); k < cap; k++, s = (s + 1) & (cap - 1))
        if (!t[s].valid || t[s].ip == ip) return &t[s];
    return NULL;
}

/* ndp_update, src/ndp_table.c:39-65 */
static upe_ndp_entry_t *ndp_slot(upe_ndp_entry_t *t, size_t cap, const uint8_t ip[16]) {
    const size_t home = ld_le32(ip) ^ ld_le32(ip + 4) ^ ld_le32(ip + 8) ^ ld_le32(ip + 12);
    for (size_t k = 0, s = home & (cap - 1); k < cap; k++, s = (s + 1) & (cap - 1))
        if (!t[s].valid || memcmp(t[s].ip, ip, 16) == 0) return &t[s];
    return NULL;
}

int upe_neigh_apply_writes(upe_arp_entry_t *arp, size_t arp_capacity, upe_ndp_entry_t *ndp,
                           size_t ndp_capacity, const upe_ctrl_write_t *writes, size_t count,
                           int64_t now, size_t *applied) {
    if ((arp_capacity & (arp_capacity - 1)) != 0 || (ndp_capacity & (ndp_capacity - 1)) != 0)
        return host_fail("upe_neigh_apply_writes: capacity must be a power of two%.0d%s", 0, "");
    if ((arp_capacity && !arp) || (ndp_capacity && !ndp) || (count && !writes))
        return host_fail("upe_neigh_apply_writes: null argument%.0d%s", 0, "");
    for (size_t k = 0; k < count; k++)
        if (writes[k].kind != UPE_CW_ARP && writes[k].kind != UPE_CW_NDP)
            return host_fail("upe_neigh_apply_writes: record %d has an unknown kind%s", (int)k, "");
    size_t done = 0;
    for (size_t k = 0; k < count; k++) {
        const upe_ctrl_write_t *w = &writes[k];
        if (w->kind == UPE_CW_ARP) {
            if (!arp_capacity) continue;
            done++;
            const uint32_t ip = ld_le32(w->ip);
            upe_arp_entry_t *e = arp_slot(arp, arp_capacity, ip);
            if (!e) continue;
            if (!e->valid) {
                e->valid = true;
                e->ip = ip;
            }
            memcpy(e->mac, w->mac, 6);
            e->update_at = now;
        } else {
            if (!ndp_capacity) continue;
            done++;
            upe_ndp_entry_t *e = ndp_slot(ndp, ndp_capacity, w->ip);
            if (!e) continue;
            if (!e->valid) {
                e->valid = true;
                memcpy(e->ip, w->ip, 16);
            }
            memcpy(e->mac, w->mac, 6);
            e->update_at = now;
        }
    }
    if (applied) *applied = done;
    return 0;
}

/* ---- latency histogram ------------------------------------------------------------------ */

static const uint64_t k_latency_bounds[UPE_LATENCY_BUCKETS] = {UPE_LATENCY_BOUNDS};

/* finite and > 0 (a NaN fails the first comparison, an infinity the second) */
static int latency_cpn_ok(double cycles_per_ns) {
    return cycles_per_ns > 0.0 && cycles_per_ns <= DBL_MAX;
}

/* (uint64_t)x for x >= 0, saturating where the plain cast is undefined */
static uint64_t latency_trunc(double x) {
    return x >= 18446744073709551616.0 ? UINT64_MAX : (uint64_t)x;
}

static void latency_sample(upe_latency_hist_t *h, uint64_t cycles, double cycles_per_ns) {
    const uint64_t ns = latency_trunc((double)cycles / cycles_per_ns);
    int b = 0; /* the first bucket whose bound ns is strictly below, else the last */
    while (b < UPE_LATENCY_BUCKETS - 1 && ns >= k_latency_bounds[b]) b++;
    h->buckets[b] += 1;
    h->total_count += 1;
    h->sum_ns += ns; /* modulo 2^64 */
    h->min_ns = ns < h->min_ns ? ns : h->min_ns;
    h->max_ns = ns > h->max_ns ? ns : h->max_ns;
}

void upe_latency_init(upe_latency_hist_t *h) {
    memset(h, 0, sizeof *h);
    h->min_ns = UPE_LATENCY_MIN_INIT;
}

int upe_latency_record(upe_latency_hist_t *h, uint64_t cycles, double cycles_per_ns) {
    if (!h) return host_fail("upe_latency_record: null histogram%.0d%s", 0, "");
    if (!latency_cpn_ok(cycles_per_ns))
        return host_fail("upe_latency_record: cycles_per_ns must be finite and > 0%.0d%s", 0, "");
    latency_sample(h, cycles, cycles_per_ns);
    return 0;
}

uint64_t upe_latency_percentile(const upe_latency_hist_t *h, double percentile) {
    if (h->total_count == 0) return 0;
    const double want = percentile * (double)h->total_count;
    const uint64_t target = want > 0.0 ? latency_trunc(want) : 0; /* NaN: 0 */
    /* the first bucket at which the running count reaches the target, else the last */
    uint64_t seen = h->buckets[0];
    int b = 0;
    while (seen < target && b < UPE_LATENCY_BUCKETS - 1) seen += h->buckets[++b];
    return k_latency_bounds[b];
}

void upe_latency_merge(upe_latency_hist_t *dst, const upe_latency_hist_t *src) {
    for (int i = 0; i < UPE_LATENCY_BUCKETS; i++) dst->buckets[i] += src->buckets[i];
    dst->total_count += src->total_count;
    dst->sum_ns += src->sum_ns;
    if (src->min_ns < dst->min_ns) dst->min_ns = src->min_ns;
    if (src->max_ns > dst->max_ns) dst->max_ns = src->max_ns;
}

int upe_latency_record_batch(upe_latency_hist_t *h, const uint64_t *timestamps,
                             const uint32_t *verdicts, size_t n, uint64_t now,
                             double cycles_per_ns) {
    if (!h || (n && !timestamps))
        return host_fail("upe_latency_record_batch: null argument%.0d%s", 0, "");
    if (!latency_cpn_ok(cycles_per_ns))
        return host_fail("upe_latency_record_batch: cycles_per_ns must be finite and > 0%.0d%s", 0,
                         "");
    for (size_t k = 0; k < n; k++) {
        if (timestamps[k] == 0) continue;
        if (verdicts && UPE_VERDICT_CODE(verdicts[k]) == UPE_V_CONSUMED) continue;
        latency_sample(h, now - timestamps[k], cycles_per_ns);
    }
    return 0;
}
