// The rule compiler (upe_amd/csrc/upe_rules.cpp) under the host sanitizers, stand-alone:
// `make -C upe_amd/csrc rules-san` builds this file with it (-fsanitize=address,undefined) and
// runs it.  Deterministic tables go through upe_rules_compile / upe_rules_image_free, and
// upe_rules_match_host is checked against a plain first-match loop over the rules (what the
// reference's rule_table_match does over match_rule, src/rule_table.c:76-91,163-176).
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/upe_gpu.h"

// the library's error slot, which upe_gpu.hip owns in the library
static char g_msg[256];
extern "C" int upe_gpu_set_last_error(const char* msg) {
    snprintf(g_msg, sizeof g_msg, "%s", msg ? msg : "");
    return -1;
}

static uint32_t g_x = 0x2545F491u;
static uint32_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 17; g_x ^= g_x << 5; return g_x; }

static bool field_ok(uint32_t key, uint32_t value, uint32_t mask) { return ((key ^ value) & mask) == 0; }
static bool addr_ok(const upe_ip_addr_t& k, const upe_ip_addr_t& v, const upe_ip_addr_t& m, int ver) {
    if (ver == 4) return field_ok(k.v4, v.v4, m.v4);
    for (int j = 0; j < 16; ++j)
        if (!field_ok(k.v6[j], v.v6[j], m.v6[j])) return false;
    return true;
}
static int64_t first_match(const std::vector<upe_rule_t>& rules, const upe_flow_key_t& k) {
    for (size_t i = 0; i < rules.size(); ++i) {
        const upe_rule_t& r = rules[i];
        if (field_ok(k.ip_ver, r.ip_ver, r.ip_ver ? 0xFF : 0) &&
            field_ok(k.protocol, r.protocol, r.protocol ? 0xFF : 0) &&
            field_ok(k.src_port, r.src_port, r.src_port ? 0xFFFF : 0) &&
            field_ok(k.dst_port, r.dst_port, r.dst_port ? 0xFFFF : 0) &&
            addr_ok(k.src_ip, r.src_ip, r.src_mask, k.ip_ver) &&
            addr_ok(k.dst_ip, r.dst_ip, r.dst_mask, k.ip_ver))
            return (int64_t)i;
    }
    return -1;
}

// `count` rules in priority order.  exact: IPv4 5-tuples under four mask signatures (a source
// address that is exact or wild, a source port that is set or wild); otherwise versions 0 / 4 / 6,
// masks of any shape (not only prefixes), fields wild about half the time.
static std::vector<upe_rule_t> table(size_t count, bool exact) {
    std::vector<upe_rule_t> t(count);
    for (size_t i = 0; i < count; ++i) {
        upe_rule_t& r = t[i];
        memset(&r, 0, sizeof r);
        r.priority = (uint32_t)i;
        r.rule_id = (uint32_t)i;
        r.action.type = (int32_t)(rnd() % 3);
        r.ip_ver = exact ? 4 : (uint8_t)(rnd() % 3 == 0 ? 0 : rnd() % 2 ? 4 : 6);
        r.protocol = exact || rnd() % 2 ? (uint8_t)(rnd() % 2 ? 6 : 17) : 0;
        r.src_port = (exact ? i % 2 : rnd() % 2) ? (uint16_t)(1 + rnd() % 65535) : 0;
        r.dst_port = exact || rnd() % 2 ? (uint16_t)(1 + rnd() % 1024) : 0;
        const int bytes = r.ip_ver == 4 ? 4 : 16;
        for (int j = 0; j < bytes; ++j) {
            r.src_ip.v6[j] = (uint8_t)rnd();
            r.dst_ip.v6[j] = (uint8_t)rnd();
            r.src_mask.v6[j] = exact ? (i % 4 < 2 ? 0xFF : 0) : (uint8_t)(rnd() % 3 ? rnd() & rnd() : 0);
            r.dst_mask.v6[j] = exact ? 0xFF : (uint8_t)(rnd() % 3 ? rnd() | rnd() : 0);
        }
    }
    return t;
}

// A key cut from rule r's own values; the bits the rule leaves free are zero, one or random.
static upe_flow_key_t key_of(const upe_rule_t& r) {
    const uint32_t mode = rnd() % 3;
    auto fill = [&]() { return mode == 0 ? 0u : mode == 1 ? ~0u : rnd(); };
    upe_flow_key_t k;
    memset(&k, 0, sizeof k);
    k.ip_ver = r.ip_ver ? r.ip_ver : (uint8_t)(rnd() % 2 ? 4 : 6);
    k.protocol = r.protocol ? r.protocol : (uint8_t)fill();
    k.src_port = r.src_port ? r.src_port : (uint16_t)fill();
    k.dst_port = r.dst_port ? r.dst_port : (uint16_t)fill();
    for (int j = 0; j < (k.ip_ver == 4 ? 4 : 16); ++j) {
        k.src_ip.v6[j] = (uint8_t)((r.src_ip.v6[j] & r.src_mask.v6[j]) | (fill() & ~r.src_mask.v6[j]));
        k.dst_ip.v6[j] = (uint8_t)((r.dst_ip.v6[j] & r.dst_mask.v6[j]) | (fill() & ~r.dst_mask.v6[j]));
    }
    return k;
}

static int run(const char* name, size_t count, bool exact, size_t nkeys) {
    const std::vector<upe_rule_t> rules = table(count, exact);
    upe_rule_image_t* im = upe_rules_compile(rules.data(), count, count);
    if (!im) return fprintf(stderr, "%s: upe_rules_compile: %s\n", name, g_msg), 1;
    upe_rules_image_free(im);
    std::vector<upe_flow_key_t> keys(nkeys);
    for (auto& k : keys) k = key_of(rules[rnd() % count]);
    std::vector<int64_t> out(nkeys, -2);
    upe_rule_index_info_t info;
    if (nkeys && upe_rules_match_host(rules.data(), count, keys.data(), nkeys, out.data(), &info) != 0)
        return fprintf(stderr, "%s: upe_rules_match_host: %s\n", name, g_msg), 1;
    size_t matched = 0;
    for (size_t i = 0; i < nkeys; ++i) {
        const int64_t want = first_match(rules, keys[i]);
        if (out[i] != want)
            return fprintf(stderr, "%s: key %zu: rule %lld, first match %lld\n", name, i,
                           (long long)out[i], (long long)want), 1;
        matched += want >= 0;
    }
    printf("%s: %zu rules compiled", name, count);
    if (nkeys) printf("; %zu keys agree with the first-match loop (%zu matched)", nkeys, matched);
    printf("\n");
    return 0;
}

int main() {
    return run("small table", 8, false, 4000) || run("family lists and tree", 200, false, 4000) ||
           run("tuple-space index", 2048, true, 0);
}
