// scanner.inc — the JSON scanner of the watch decoder. Unity-build fragment,
// #included into kwcore.cpp at the top of its anonymous namespace; nothing
// here touches Python, so the fragments over it that do not either
// (findings.inc) also build into a stand-alone program (tools/findings_check.cpp).
//
// Byte spans of raw JSON tokens, string escapes, the structural scanner
// (Parser: scalar, AVX2 and AVX-512BW forms) and the pod walkers built on it:
// the full parse, the filter-first light parse and materialize().

// ----------------------------------------------------------------------------- spans

struct Span {
    const char* p = nullptr;  // raw JSON token (strings include their quotes)
    size_t n = 0;
    bool present() const { return p != nullptr; }
    bool is_null() const { return p && n == 4 && std::memcmp(p, "null", 4) == 0; }
    bool is_string() const { return p && n >= 2 && p[0] == '"'; }
};

struct Condition { Span type, status, reason, message; };
struct CStatus { Span name, ready, restart_count, state; };
struct Container { Span name, image; };

struct PodSpans {
    bool meta_present = false;
    Span name, ns, uid, rv, labels, annotations, ctime, owners;
    Span pod_ip, host_ip, start_time, qos;  // watcher.payload_extra_fields
    // metadata.deletionTimestamp / deletionGracePeriodSeconds / finalizers:
    // watcher.alerts.terminating and the extra field termination (findings.inc)
    Span del_time, del_grace, finalizers;
    bool spec_present = false;
    Span node_name;
    std::vector<Container> containers;
    bool status_present = false;
    Span phase;
    std::vector<Condition> conditions;
    std::vector<CStatus> cstatuses;
    bool deferred = false;             // parse_pod_light: spec/arrays not walked yet
    Span spec_raw, cond_raw, cstat_raw;
    Span init_raw;  // status.initContainerStatuses, never walked but by the findings (findings.inc)
    void clear() {
        meta_present = spec_present = status_present = deferred = false;
        name = ns = uid = rv = labels = annotations = ctime = node_name = phase = Span();
        owners = pod_ip = host_ip = start_time = qos = Span();
        del_time = del_grace = finalizers = Span();
        spec_raw = cond_raw = cstat_raw = init_raw = Span();
        containers.clear();
        conditions.clear();
        cstatuses.clear();
    }
};

struct ParseError {
    const char* msg;
};

// ----------------------------------------------------------------------------- string escapes

void append_utf8_codepoint(std::string& o, uint32_t cp) {
    if (cp < 0x80) {
        o.push_back((char)cp);
    } else if (cp < 0x800) {
        o.push_back((char)(0xC0 | (cp >> 6)));
        o.push_back((char)(0x80 | (cp & 0x3F)));
    } else if (cp < 0x10000) {
        o.push_back((char)(0xE0 | (cp >> 12)));
        o.push_back((char)(0x80 | ((cp >> 6) & 0x3F)));
        o.push_back((char)(0x80 | (cp & 0x3F)));
    } else {
        o.push_back((char)(0xF0 | (cp >> 18)));
        o.push_back((char)(0x80 | ((cp >> 12) & 0x3F)));
        o.push_back((char)(0x80 | ((cp >> 6) & 0x3F)));
        o.push_back((char)(0x80 | (cp & 0x3F)));
    }
}

int hexval(char c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

bool read_u4(const char* p, const char* e, uint32_t& out) {
    if (e - p < 4) return false;
    uint32_t v = 0;
    for (int i = 0; i < 4; ++i) {
        int h = hexval(p[i]);
        if (h < 0) return false;
        v = (v << 4) | (uint32_t)h;
    }
    out = v;
    return true;
}

// The text of a JSON string's inside p..e (no quotes) with its escapes decoded
// as json.loads decodes them; a lone surrogate becomes its three-byte form
// (what "surrogatepass" reads back). Cold: callers come here only for a span
// that holds a backslash.
void json_unescape(std::string& o, const char* p, const char* e) {
    while (p < e) {
        char c = *p++;
        if (c != '\\') {
            o.push_back(c);
            continue;
        }
        if (p >= e) break;
        char d = *p++;
        switch (d) {
            case '"': o.push_back('"'); break;
            case '\\': o.push_back('\\'); break;
            case '/': o.push_back('/'); break;
            case 'b': o.push_back('\b'); break;
            case 'f': o.push_back('\f'); break;
            case 'n': o.push_back('\n'); break;
            case 'r': o.push_back('\r'); break;
            case 't': o.push_back('\t'); break;
            case 'u': {
                uint32_t cp;
                if (!read_u4(p, e, cp)) { o.push_back('?'); break; }
                p += 4;
                if (cp >= 0xD800 && cp <= 0xDBFF && e - p >= 6 && p[0] == '\\' && p[1] == 'u') {
                    uint32_t lo;
                    if (read_u4(p + 2, e, lo) && lo >= 0xDC00 && lo <= 0xDFFF) {
                        cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00);
                        p += 6;
                    }
                }
                append_utf8_codepoint(o, cp);
                break;
            }
            default: o.push_back(d);
        }
    }
}

// ----------------------------------------------------------------------------- scanner

class Parser {
  public:
    Parser(const char* b, const char* e) : p_(b), end_(e) {}
    const char* p_;
    const char* end_;
    bool esc_ = false;    // set by the string scanners when they meet a backslash (key() reads it)
    std::string keybuf_;  // the decoded text of a key spelled with escapes

    [[noreturn]] void fail(const char* m) { throw ParseError{m}; }

    inline void ws() {
        while (p_ < end_ && (*p_ == ' ' || *p_ == '\n' || *p_ == '\r' || *p_ == '\t')) ++p_;
    }
    inline char peek() {
        ws();
        if (p_ >= end_) fail("unexpected end of input");
        return *p_;
    }
    inline void expect(char c) {
        if (peek() != c) fail("unexpected character");
        ++p_;
    }

    // Returns pointer one past the closing quote of the string starting at p_ ('"').
    inline const char* string_end(const char* s) {
        ++s;  // opening quote
#if defined(__x86_64__)
        if (use_avx2) return string_end_avx2(s);
#endif
        while (s < end_) {
            char c = *s;
            if (c == '"') return s + 1;
            if (c == '\\') {
                esc_ = true;
                s += 2;
                continue;
            }
            ++s;
        }
        fail("unterminated string");
    }

#if defined(__x86_64__)
    static bool use_avx2;
    static bool use_avx512;
    __attribute__((target("avx2,bmi,bmi2"))) const char* string_end_avx2(const char* s) {
        const __m256i q = _mm256_set1_epi8('"');
        const __m256i bs = _mm256_set1_epi8('\\');
        while (s + 32 <= end_) {
            __m256i v = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(s));
            uint32_t mq = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, q));
            uint32_t mb = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, bs));
            if (mb == 0) {
                if (mq) return s + __builtin_ctz(mq) + 1;
                s += 32;
                continue;
            }
            uint32_t first_b = __builtin_ctz(mb);
            if (mq && (uint32_t)__builtin_ctz(mq) < first_b) return s + __builtin_ctz(mq) + 1;
            esc_ = true;
            s += first_b + 2;  // skip the escape pair, rescan from there
        }
        while (s < end_) {
            char c = *s;
            if (c == '"') return s + 1;
            if (c == '\\') {
                esc_ = true;
                s += 2;
                continue;
            }
            ++s;
        }
        fail("unterminated string");
    }

    // Skip a balanced {...} or [...] starting at s (the opener), 64 bytes per
    // step: structural-character bitmasks from two AVX2 compares, escaped
    // quotes removed with the odd-backslash-run rule, string interiors masked
    // with a carry-less-multiply prefix XOR, and the bracket depth advanced
    // by popcounts; bits are only walked one by one in the block where the
    // depth can return to zero.
    static inline __attribute__((target("avx2"))) uint64_t mask64(__m256i lo, __m256i hi, __m256i c) {
        uint32_t a = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(lo, c));
        uint32_t b = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(hi, c));
        return (uint64_t)a | ((uint64_t)b << 32);
    }

    static inline uint64_t escaped_mask(uint64_t backslash, uint64_t& prev_escaped) {
        const uint64_t even = 0x5555555555555555ULL;
        backslash &= ~prev_escaped;
        uint64_t follows = (backslash << 1) | prev_escaped;
        uint64_t odd_starts = backslash & ~even & ~follows;
        uint64_t seq_even;
        prev_escaped = __builtin_add_overflow(odd_starts, backslash, &seq_even) ? 1 : 0;
        uint64_t invert = seq_even << 1;
        return (even ^ invert) & follows;
    }

    __attribute__((target("avx2,bmi,bmi2,pclmul,popcnt"))) const char* skip_container_blocks(const char* s) {
        uint64_t prev_escaped = 0, prev_in_string = 0;
        int64_t depth = 0;
        const char* p = s;
        alignas(32) char tail[64];
        const __m256i vq = _mm256_set1_epi8('"'), vb = _mm256_set1_epi8('\\');
        const __m256i vob = _mm256_set1_epi8('{'), vcb = _mm256_set1_epi8('}');
        const __m256i v20 = _mm256_set1_epi8(0x20);
        while (p < end_) {
            size_t avail = (size_t)(end_ - p);
            const char* blk = p;
            uint64_t valid = ~0ULL;
            if (avail < 64) {
                std::memset(tail, ' ', sizeof tail);
                std::memcpy(tail, p, avail);
                blk = tail;
                valid = (1ULL << avail) - 1;
            }
            __m256i lo = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(blk));
            __m256i hi = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(blk + 32));
            uint64_t quotes = mask64(lo, hi, vq) & ~escaped_mask(mask64(lo, hi, vb), prev_escaped);
            uint64_t in_str = (uint64_t)_mm_cvtsi128_si64(
                _mm_clmulepi64_si128(_mm_set_epi64x(0, (long long)quotes), _mm_set1_epi8((char)0xFF), 0));
            in_str ^= prev_in_string;
            prev_in_string = (uint64_t)((int64_t)in_str >> 63);
            // '{'|0x20 == '['|0x20 == '{' and '}'|0x20 == ']'|0x20 == '}': one compare per bracket kind
            const __m256i lo20 = _mm256_or_si256(lo, v20), hi20 = _mm256_or_si256(hi, v20);
            uint64_t open = mask64(lo20, hi20, vob) & ~in_str & valid;
            uint64_t close = mask64(lo20, hi20, vcb) & ~in_str & valid;
            int64_t nclose = __builtin_popcountll(close);
            if (depth > nclose) {
                depth += __builtin_popcountll(open) - nclose;
            } else {
                uint64_t m = open | close;
                while (m) {
                    int i = __builtin_ctzll(m);
                    if ((open >> i) & 1) {
                        ++depth;
                    } else if (--depth == 0) {
                        return p + i + 1;
                    }
                    m &= m - 1;
                }
            }
            p += avail < 64 ? avail : 64;
        }
        fail("unterminated container");
    }

    // AVX-512BW form of the same block scanner (Zen 4/5 and recent Xeons run
    // 512-bit compares at full width): one load and four compares yield the
    // 64-bit quote/backslash/open/close masks directly in mask registers, the
    // escape pass is skipped for blocks with no backslash, and the final
    // partial block is a fault-suppressing masked load instead of a copy.
    __attribute__((target("avx512f,avx512bw,bmi,bmi2,pclmul,popcnt"))) const char* skip_container_512(
        const char* s) {
        uint64_t prev_escaped = 0, prev_in_string = 0;
        int64_t depth = 0;
        const char* p = s;
        const __m512i vq = _mm512_set1_epi8('"'), vb = _mm512_set1_epi8('\\');
        const __m512i vo = _mm512_set1_epi8('{'), vc = _mm512_set1_epi8('}'), v20 = _mm512_set1_epi8(0x20);
        while (p < end_) {
            size_t avail = (size_t)(end_ - p);
            uint64_t valid = ~0ULL;
            __m512i v;
            if (avail >= 64) {
                v = _mm512_loadu_si512(reinterpret_cast<const void*>(p));
            } else {
                valid = (1ULL << avail) - 1;
                v = _mm512_maskz_loadu_epi8(valid, p);
            }
            uint64_t quotes = _mm512_cmpeq_epi8_mask(v, vq);
            uint64_t bs = _mm512_cmpeq_epi8_mask(v, vb);
            if (bs | prev_escaped) quotes &= ~escaped_mask(bs, prev_escaped);
            uint64_t in_str = (uint64_t)_mm_cvtsi128_si64(
                _mm_clmulepi64_si128(_mm_set_epi64x(0, (long long)quotes), _mm_set1_epi8((char)0xFF), 0));
            in_str ^= prev_in_string;
            prev_in_string = (uint64_t)((int64_t)in_str >> 63);
            const __m512i f = _mm512_or_si512(v, v20);
            uint64_t open = _mm512_cmpeq_epi8_mask(f, vo) & ~in_str & valid;
            uint64_t close = _mm512_cmpeq_epi8_mask(f, vc) & ~in_str & valid;
            int64_t nclose = __builtin_popcountll(close);
            if (depth > nclose) {
                depth += __builtin_popcountll(open) - nclose;
            } else {
                uint64_t m = open | close;
                while (m) {
                    int i = __builtin_ctzll(m);
                    if ((open >> i) & 1) {
                        ++depth;
                    } else if (--depth == 0) {
                        return p + i + 1;
                    }
                    m &= m - 1;
                }
            }
            p += avail < 64 ? avail : 64;
        }
        fail("unterminated container");
    }

    __attribute__((target("avx2,bmi,bmi2"))) const char* skip_container_avx2(const char* s) {
        int depth = 0;
        const __m256i q = _mm256_set1_epi8('"');
        const __m256i ob = _mm256_set1_epi8('{');
        const __m256i cb = _mm256_set1_epi8('}');
        const __m256i os = _mm256_set1_epi8('[');
        const __m256i cs = _mm256_set1_epi8(']');
        while (s + 32 <= end_) {
            __m256i v = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(s));
            uint32_t m = (uint32_t)_mm256_movemask_epi8(
                _mm256_or_si256(_mm256_or_si256(_mm256_cmpeq_epi8(v, q), _mm256_cmpeq_epi8(v, ob)),
                                _mm256_or_si256(_mm256_cmpeq_epi8(v, cb),
                                                _mm256_or_si256(_mm256_cmpeq_epi8(v, os),
                                                                _mm256_cmpeq_epi8(v, cs)))));
            const char* next = s + 32;
            while (m) {
                uint32_t i = __builtin_ctz(m);
                const char* c = s + i;
                char ch = *c;
                if (ch == '"') {
                    const char* after = string_end_avx2(c + 1);
                    if (after > s + 32) {
                        next = after;
                        m = 0;
                        break;
                    }
                    // clear bits up to and including the closing quote
                    uint32_t upto = (uint32_t)(after - s);
                    m = upto >= 32 ? 0 : (m & ~((1u << upto) - 1u));
                    if (upto >= 32) {
                        next = after;
                        break;
                    }
                    continue;
                }
                if (ch == '{' || ch == '[') {
                    ++depth;
                } else {
                    if (--depth == 0) return c + 1;
                }
                m &= m - 1;
            }
            s = next;
        }
        return skip_container_scalar(s, depth);
    }
#endif

    const char* skip_container_scalar(const char* s, int depth) {
        while (s < end_) {
            char c = *s;
            if (c == '"') {
                s = string_end_scalar(s + 1);
                continue;
            }
            if (c == '{' || c == '[') {
                ++depth;
            } else if (c == '}' || c == ']') {
                if (--depth == 0) return s + 1;
            }
            ++s;
        }
        fail("unterminated container");
    }

    const char* string_end_scalar(const char* s) {
        while (s < end_) {
            char c = *s;
            if (c == '"') return s + 1;
            if (c == '\\') {
                esc_ = true;
                s += 2;
                continue;
            }
            ++s;
        }
        fail("unterminated string");
    }

    // Skip any JSON value at p_ and return its raw span.
    Span value() {
        char c = peek();
        Span sp;
        sp.p = p_;
        if (c == '"') {
            p_ = string_end(p_);
        } else if (c == '{' || c == '[') {
#if defined(__x86_64__)
            p_ = use_avx512 ? skip_container_512(p_)
                 : use_avx2 ? skip_container_blocks(p_)
                            : skip_container_scalar(p_, 0);
#else
            p_ = skip_container_scalar(p_, 0);
#endif
        } else {
            while (p_ < end_) {
                char d = *p_;
                if (d == ',' || d == '}' || d == ']' || d == ' ' || d == '\n' || d == '\r' || d == '\t') break;
                ++p_;
            }
            if (p_ == sp.p) fail("empty value");
        }
        sp.n = (size_t)(p_ - sp.p);
        return sp;
    }

    // Read an object key (without quotes) and consume the following ':'. A key
    // spelled with escapes ("name") is the key json.loads reads: it is
    // decoded into keybuf_, which holds until the next key() of this parser.
    inline void key(const char*& k, size_t& kn) {
        if (peek() != '"') fail("expected key");
        const char* s = p_ + 1;
        esc_ = false;
        p_ = string_end(p_);
        k = s;
        kn = (size_t)(p_ - 1 - s);
        if (__builtin_expect(esc_, 0)) escaped_key(k, kn);
        expect(':');
    }

    __attribute__((noinline, cold)) void escaped_key(const char*& k, size_t& kn) {
        keybuf_.clear();
        json_unescape(keybuf_, k, k + kn);
        k = keybuf_.data();
        kn = keybuf_.size();
    }

    // Iterate an object: f(key, keylen) must consume the value.
    template <class F>
    void object(F&& f) {
        expect('{');
        if (peek() == '}') {
            ++p_;
            return;
        }
        while (true) {
            const char* k;
            size_t kn;
            key(k, kn);
            f(k, kn);
            char c = peek();
            ++p_;
            if (c == '}') return;
            if (c != ',') fail("expected , or }");
        }
    }

    template <class F>
    void array(F&& f) {
        expect('[');
        if (peek() == ']') {
            ++p_;
            return;
        }
        while (true) {
            f();
            char c = peek();
            ++p_;
            if (c == ']') return;
            if (c != ',') fail("expected , or ]");
        }
    }

    bool null_here() {
        if (peek() == 'n' && end_ - p_ >= 4 && std::memcmp(p_, "null", 4) == 0) {
            p_ += 4;
            return true;
        }
        return false;
    }
};

#if defined(__x86_64__)
bool Parser::use_avx2 = false;
bool Parser::use_avx512 = false;

bool simd_supported() {
    __builtin_cpu_init();
    return __builtin_cpu_supports("avx2") && __builtin_cpu_supports("bmi2") &&
           __builtin_cpu_supports("pclmul") && __builtin_cpu_supports("popcnt");
}

bool avx512_supported() {
    __builtin_cpu_init();
    return simd_supported() && __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512bw");
}
#endif

#define KEYIS(lit) (kn == sizeof(lit) - 1 && std::memcmp(k, lit, sizeof(lit) - 1) == 0)

void parse_metadata(Parser& P, PodSpans& S) {
    // a repeated "metadata" key replaces the first one whole (json.loads: the last key wins)
    S.meta_present = false;
    S.name = S.ns = S.uid = S.rv = S.labels = S.annotations = S.ctime = S.owners = Span();
    S.del_time = S.del_grace = S.finalizers = Span();
    if (P.null_here()) return;
    S.meta_present = true;
    P.object([&](const char* k, size_t kn) {
        switch (kn) {
            case 3:
                if (KEYIS("uid")) { S.uid = P.value(); return; }
                break;
            case 4:
                if (KEYIS("name")) { S.name = P.value(); return; }
                break;
            case 6:
                if (KEYIS("labels")) { S.labels = P.value(); return; }
                break;
            case 9:
                if (KEYIS("namespace")) { S.ns = P.value(); return; }
                break;
            case 10:
                if (KEYIS("finalizers")) { S.finalizers = P.value(); return; }
                break;
            case 11:
                if (KEYIS("annotations")) { S.annotations = P.value(); return; }
                break;
            case 15:
                if (KEYIS("resourceVersion")) { S.rv = P.value(); return; }
                if (KEYIS("ownerReferences")) { S.owners = P.value(); return; }
                break;
            case 17:
                if (KEYIS("creationTimestamp")) { S.ctime = P.value(); return; }
                if (KEYIS("deletionTimestamp")) { S.del_time = P.value(); return; }
                break;
            case 26:
                if (KEYIS("deletionGracePeriodSeconds")) { S.del_grace = P.value(); return; }
                break;
        }
        P.value();
    });
}

// "metadata" present but not an object or null: as absent (the Python engine reads it as {})
void parse_metadata_absent(PodSpans& S) {
    S.meta_present = false;
    S.name = S.ns = S.uid = S.rv = S.labels = S.annotations = S.ctime = S.owners = Span();
    S.del_time = S.del_grace = S.finalizers = Span();
}

void parse_containers(Parser& P, PodSpans& S) {
    S.containers.clear();  // a repeated key replaces the list (json.loads: the last key wins)
    if (P.null_here()) return;
    if (P.peek() != '[') { P.value(); return; }
    P.array([&]() {
        if (P.peek() != '{') { P.value(); return; }
        Container c;
        P.object([&](const char* k, size_t kn) {
            if (KEYIS("name")) c.name = P.value();
            else if (KEYIS("image")) c.image = P.value();
            else P.value();
        });
        S.containers.push_back(c);
    });
}

void parse_conditions(Parser& P, PodSpans& S) {
    S.conditions.clear();  // a repeated key replaces the list (json.loads: the last key wins)
    if (P.null_here()) return;
    if (P.peek() != '[') { P.value(); return; }
    P.array([&]() {
        if (P.peek() != '{') { P.value(); return; }
        Condition c;
        P.object([&](const char* k, size_t kn) {
            if (KEYIS("type")) c.type = P.value();
            else if (KEYIS("status")) c.status = P.value();
            else if (KEYIS("reason")) c.reason = P.value();
            else if (KEYIS("message")) c.message = P.value();
            else P.value();
        });
        S.conditions.push_back(c);
    });
}

void parse_cstatuses(Parser& P, PodSpans& S) {
    S.cstatuses.clear();  // a repeated key replaces the list (json.loads: the last key wins)
    if (P.null_here()) return;
    if (P.peek() != '[') { P.value(); return; }
    P.array([&]() {
        if (P.peek() != '{') { P.value(); return; }
        CStatus c;
        P.object([&](const char* k, size_t kn) {
            if (KEYIS("name")) c.name = P.value();
            else if (KEYIS("ready")) c.ready = P.value();
            else if (KEYIS("restartCount")) c.restart_count = P.value();
            else if (KEYIS("state")) c.state = P.value();
            else P.value();
        });
        S.cstatuses.push_back(c);
    });
}

void reset_spec(PodSpans& S) {
    S.spec_present = false;
    S.node_name = S.spec_raw = Span();
    S.containers.clear();
}

void reset_status(PodSpans& S) {
    S.status_present = false;
    S.phase = S.pod_ip = S.host_ip = S.start_time = S.qos = S.cond_raw = S.cstat_raw = S.init_raw = Span();
    S.conditions.clear();
    S.cstatuses.clear();
}

void parse_spec(Parser& P, PodSpans& S) {
    if (P.null_here()) return;
    S.spec_present = true;
    P.object([&](const char* k, size_t kn) {
        if (KEYIS("nodeName")) S.node_name = P.value();
        else if (KEYIS("containers")) parse_containers(P, S);
        else P.value();
    });
}

// status scalars for watcher.payload_extra_fields (a few length-gated compares),
// and the raw initContainerStatuses for the container failure findings
bool status_scalar(Parser& P, PodSpans& S, const char* k, size_t kn) {
    switch (kn) {
        case 5:
            if (KEYIS("podIP")) { S.pod_ip = P.value(); return true; }
            break;
        case 6:
            if (KEYIS("hostIP")) { S.host_ip = P.value(); return true; }
            break;
        case 8:
            if (KEYIS("qosClass")) { S.qos = P.value(); return true; }
            break;
        case 9:
            if (KEYIS("startTime")) { S.start_time = P.value(); return true; }
            break;
        case 21:
            if (KEYIS("initContainerStatuses")) { S.init_raw = P.value(); return true; }
            break;
    }
    return false;
}

void parse_status(Parser& P, PodSpans& S) {
    if (P.null_here()) return;
    S.status_present = true;
    P.object([&](const char* k, size_t kn) {
        if (KEYIS("phase")) S.phase = P.value();
        else if (KEYIS("conditions")) {
            P.peek();  // the raw span too, as below: the unready-since walks it for the transition time
            const char* start = P.p_;
            parse_conditions(P, S);
            S.cond_raw = Span{start, (size_t)(P.p_ - start)};
        } else if (KEYIS("containerStatuses")) {
            P.peek();  // (skips blanks) the raw span too, as the light parse keeps it: findings.inc walks it
            const char* start = P.p_;
            parse_cstatuses(P, S);
            S.cstat_raw = Span{start, (size_t)(P.p_ - start)};
        } else if (!status_scalar(P, S, k, kn)) P.value();
    });
}

void parse_pod(Parser& P, PodSpans& S) {
    P.object([&](const char* k, size_t kn) {
        if (KEYIS("metadata")) {
            if (P.peek() == '{' || P.peek() == 'n') {
                parse_metadata(P, S);
            } else {
                P.value();
                parse_metadata_absent(S);
            }
        } else if (KEYIS("spec")) {
            reset_spec(S);
            if (P.peek() == '{' || P.peek() == 'n') parse_spec(P, S); else P.value();
        } else if (KEYIS("status")) {
            reset_status(S);
            if (P.peek() == '{' || P.peek() == 'n') parse_status(P, S); else P.value();
        } else {
            P.value();
        }
    });
}

// Filter-first variant for the fused pipeline: everything the filters and the
// cache need (metadata, status.phase) is extracted, while spec and the two
// status arrays are only bracket-skipped by the block scanner and their raw
// spans kept; materialize() walks them later for the events that actually get
// a payload. With the critical-events filter ~4 of 5 churn events never pay
// for the container/condition walk.
void parse_status_light(Parser& P, PodSpans& S) {
    if (P.null_here()) return;
    S.status_present = true;
    P.object([&](const char* k, size_t kn) {
        if (KEYIS("phase")) S.phase = P.value();
        else if (KEYIS("conditions")) S.cond_raw = P.value();
        else if (KEYIS("containerStatuses")) S.cstat_raw = P.value();
        else if (!status_scalar(P, S, k, kn)) P.value();
    });
}

void parse_pod_light(Parser& P, PodSpans& S) {
    S.deferred = true;
    P.object([&](const char* k, size_t kn) {
        if (KEYIS("metadata")) {
            if (P.peek() == '{' || P.peek() == 'n') {
                parse_metadata(P, S);
            } else {
                P.value();
                parse_metadata_absent(S);
            }
        } else if (KEYIS("spec")) {
            reset_spec(S);
            char c = P.peek();
            if (c == '{') {
                S.spec_present = true;
                S.spec_raw = P.value();
            } else if (!P.null_here()) {
                P.value();
            }
        } else if (KEYIS("status")) {
            reset_status(S);
            if (P.peek() == '{' || P.peek() == 'n') parse_status_light(P, S); else P.value();
        } else {
            P.value();
        }
    });
}

// Walk the sub-trees parse_pod_light deferred; throws ParseError like parse_pod.
void materialize(PodSpans& S) {
    if (!S.deferred) return;
    S.deferred = false;
    if (S.spec_raw.present()) {
        Parser Q(S.spec_raw.p, S.spec_raw.p + S.spec_raw.n);
        parse_spec(Q, S);
    }
    if (S.cond_raw.present()) {
        Parser Q(S.cond_raw.p, S.cond_raw.p + S.cond_raw.n);
        parse_conditions(Q, S);
    }
    if (S.cstat_raw.present()) {
        Parser Q(S.cstat_raw.p, S.cstat_raw.p + S.cstat_raw.n);
        parse_cstatuses(Q, S);
    }
}
