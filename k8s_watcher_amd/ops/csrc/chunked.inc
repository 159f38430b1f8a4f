// chunked.inc — HTTP/1.1 chunked de-framing and NDJSON line splitting of a
// watch body: the one state machine and the one splitter under
// StreamDecoder.feed_chunked, Pipeline.feed_chunked, the reader hub's framing
// and WatchList.feed. Unity-build fragment, #included into kwcore.cpp inside
// its anonymous namespace after scanner.inc (hexval); nothing of Python here
// (check/chunked_check.cpp runs it stand-alone under the sanitizers).
//
// A stream moves between two consumers while it is live (ReaderHub's
// take_dispatch hands the pipeline's ChunkState to the hub), so there is one
// set of rules, and what differs per consumer is in its sink: which lines it
// drops, when it stops, how it reports an error.

// size line → data → CRLF ... → 0-size chunk → trailers
enum { CS_SIZE, CS_DATA, CS_DATA_END, CS_TRAILER, CS_DONE };

// 1*HEXDIG [BWS] [";" ext] in line[0..n), the value checked for overflow. The
// watch side (lenient) also takes blanks in front and the line's CR among the
// blanks behind; the clusterapi response scanner (scan_response) takes neither.
bool parse_chunk_size(const char* line, size_t n, size_t& size, bool lenient) {
    size_t v = 0;
    size_t i = 0;
    while (lenient && i < n && (line[i] == ' ' || line[i] == '\t')) ++i;
    size_t start = i;
    for (; i < n; ++i) {
        int h = hexval(line[i]);
        if (h < 0) break;
        if (v > (SIZE_MAX >> 4)) return false;
        v = (v << 4) | (size_t)h;
    }
    if (i == start) return false;
    while (i < n && (line[i] == ' ' || line[i] == '\t' || (lenient && line[i] == '\r'))) ++i;
    if (i < n && line[i] != ';') return false;
    size = v;
    return true;
}

bool parse_chunk_size(const std::string& line, size_t& size) {
    return parse_chunk_size(line.data(), line.size(), size, true);
}

// A chunked body's framing state between two reads. A default-constructed
// value is the start of a body.
struct ChunkState {
    int cstate = CS_SIZE;
    size_t cremain = 0;  // bytes left in the current chunk
    std::string line;    // chunk size / trailer line being assembled
    bool done() const { return cstate == CS_DONE; }
};

enum ChunkEnd {
    CE_MORE,      // every byte consumed, the body goes on
    CE_STOPPED,   // the sink stopped it (the data run it stopped at is consumed)
    CE_DONE,      // the terminating chunk and its trailer: end of the body, nothing after it is framed
    CE_TOO_LONG,  // a size line past 4096 bytes with no end
    CE_BAD_SIZE,  // a size line that is no chunk size (it stays in st.line)
};

constexpr size_t CHUNK_LINE_MAX = 4096;

// The text of a framing error, as every consumer but WatchList reports it
// (the reader hub through this, the others through set_chunk_error).
std::string chunk_error_text(const ChunkState& st, ChunkEnd e) {
    if (e == CE_TOO_LONG) return "chunk size line too long";
    char msg[64];
    std::snprintf(msg, sizeof msg, "bad chunk size line %.40s", st.line.c_str());
    return msg;
}

// De-frame bytes [from, to) of `base`: sink(off, len) -> bool gets every run
// of chunk-data bytes (base[off, off + len), len > 0) and returns false to
// stop. `at` is the offset after the bytes consumed — where an error or the
// end of the body was found.
template <class Sink>
inline ChunkEnd chunk_deframe(ChunkState& st, const char* base, size_t from, size_t to, size_t& at, Sink&& sink) {
    size_t i = from;
    ChunkEnd end = CE_MORE;
    while (i < to && end == CE_MORE) {
        switch (st.cstate) {
            case CS_SIZE: {
                const char* nl = (const char*)std::memchr(base + i, '\n', to - i);
                if (!nl) {
                    st.line.append(base + i, to - i);
                    i = to;
                    if (st.line.size() > CHUNK_LINE_MAX) end = CE_TOO_LONG;
                    break;
                }
                st.line.append(base + i, (size_t)(nl - (base + i)));
                i = (size_t)(nl - base) + 1;
                size_t size;
                if (!parse_chunk_size(st.line, size)) {
                    end = CE_BAD_SIZE;
                    break;
                }
                st.line.clear();
                if (size == 0) {
                    st.cstate = CS_TRAILER;
                } else {
                    st.cremain = size;
                    st.cstate = CS_DATA;
                }
                break;
            }
            case CS_DATA: {
                const size_t take = st.cremain < to - i ? st.cremain : to - i;
                if (!sink(i, take)) end = CE_STOPPED;
                i += take;
                st.cremain -= take;
                if (st.cremain == 0) st.cstate = CS_DATA_END;
                break;
            }
            case CS_DATA_END: {
                const char* nl = (const char*)std::memchr(base + i, '\n', to - i);
                if (!nl) {
                    i = to;
                    break;
                }
                i = (size_t)(nl - base) + 1;
                st.cstate = CS_SIZE;
                break;
            }
            case CS_TRAILER: {  // header lines up to the empty one
                const char* nl = (const char*)std::memchr(base + i, '\n', to - i);
                if (!nl) {
                    st.line.append(base + i, to - i);
                    i = to;
                    break;
                }
                st.line.append(base + i, (size_t)(nl - (base + i)));
                i = (size_t)(nl - base) + 1;
                const bool empty = st.line.empty() || (st.line.size() == 1 && st.line[0] == '\r');
                st.line.clear();
                if (empty) {
                    st.cstate = CS_DONE;
                    end = CE_DONE;
                }
                break;
            }
            default:  // CS_DONE
                end = CE_DONE;
        }
    }
    at = i;
    return end;
}

// What the line splitter makes of a run of body bytes (the reader hub's item
// kinds HI_LINE / HI_FRAG / HI_FRAG_END, engine.inc, are these).
enum : uint8_t {
    LN_WHOLE = 0,     // a whole line
    LN_FRAG = 1,      // bytes of a line that continues past this run
    LN_FRAG_END = 2,  // the last bytes (maybe none) of a line begun in earlier runs
};

// Split body bytes base[a, a + n) into NDJSON lines: sink(kind, off, len) ->
// bool per piece, false to stop (the rest of the run is dropped). `open`: a
// line begun in an earlier run has not ended — the caller's to keep. A
// fragment is never empty; whole lines may be (the sink drops what it wants).
template <class Sink>
inline bool split_lines(const char* base, size_t a, size_t n, bool& open, Sink&& sink) {
    size_t pos = a;
    const size_t end = a + n;
    while (pos < end) {
        const char* nl = (const char*)std::memchr(base + pos, '\n', end - pos);
        if (!nl) {
            open = true;
            return sink(LN_FRAG, pos, end - pos);
        }
        const size_t len = (size_t)(nl - base) - pos;
        const uint8_t kind = open ? LN_FRAG_END : LN_WHOLE;
        open = false;
        pos += len + 1;
        if (!sink(kind, pos - len - 1, len)) return false;
    }
    return true;
}

// The consumers that carry a split line in a string (`partial`: empty exactly
// when no line is open): append on a fragment, line(b, n, joined) and clear
// on the fragment that ends it, line(b, n, nullptr) on a whole line. `joined`
// is `partial` itself when b points into it; line() may move it away.
template <class Line>
inline bool join_line(std::string& partial, uint8_t kind, const char* b, size_t n, Line&& line) {
    if (kind == LN_WHOLE) return line(b, n, (std::string*)nullptr);
    partial.append(b, n);
    if (kind == LN_FRAG) return true;
    const bool go = line(partial.data(), partial.size(), &partial);
    partial.clear();
    return go;
}
