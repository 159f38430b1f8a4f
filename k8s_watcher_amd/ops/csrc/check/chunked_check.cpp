// chunked_check — the chunked-body framer and NDJSON line splitter
// (../chunked.inc over ../scanner.inc's hexval) as a stand-alone program, for
// a run under -fsanitize=address,undefined (scripts/chunked_check.sh). No
// Python.
//
//   chunked_check FRAMINGS.tsv
//
// FRAMINGS.tsv holds one framing per line: its name, a tab, its bytes in hex.
// Each is framed the way the string-carrying consumers do it (a ChunkState and
// a partial line, every piece in a heap block of its exact size so an overread
// is seen) whole, at every two-piece cut and one byte per feed, and the way
// the reader hub does it (one buffer that grows, bytes [from, to) framed into
// line items, the items walked afterwards) in steps of 1, 7 and all bytes.
// All of these must recover the same lines and end in the same state, or in
// the same error after the same lines; that goes to stdout, one line per
// framing: name, final state or hex of the error text, then the non-blank
// lines in hex, tab-separated.

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <string_view>
#include <vector>

#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace {

#include "../scanner.inc"
#include "../chunked.inc"

struct Out {
    std::vector<std::string> lines;
    std::string end;  // the final state, or "error " and the text
    bool operator==(const Out& o) const { return lines == o.lines && end == o.end; }
};

bool blank(const char* b, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!(b[i] == ' ' || b[i] == '\r' || b[i] == '\t' || b[i] == '\n')) return false;
    return true;
}

std::string final_state(const ChunkState& st, bool open) {
    if (st.done()) return "done";
    return "state " + std::to_string(st.cstate) + " remain " + std::to_string(st.cremain) + " open " +
           std::to_string((int)open);
}

bool keep(Out& out, const char* b, size_t n) {
    if (n && !blank(b, n)) out.lines.emplace_back(b, n);
    return true;
}

// the decoder's, the pipeline's and WatchList's way
Out feed_pieces(const std::vector<std::string>& pieces) {
    Out out;
    ChunkState st;
    std::string partial;
    for (const std::string& piece : pieces) {
        std::unique_ptr<char[]> buf(new char[piece.size() ? piece.size() : 1]);
        std::memcpy(buf.get(), piece.data(), piece.size());
        const char* data = buf.get();
        size_t at = 0;
        const ChunkEnd end = chunk_deframe(st, data, 0, piece.size(), at, [&](size_t off, size_t len) {
            bool open = !partial.empty();
            return split_lines(data, off, len, open, [&](uint8_t kind, size_t o, size_t n) {
                return join_line(partial, kind, data + o, n,
                                 [&](const char* b, size_t bn, std::string*) { return keep(out, b, bn); });
            });
        });
        if (end == CE_TOO_LONG || end == CE_BAD_SIZE) {
            out.end = "error " + chunk_error_text(st, end);
            return out;
        }
        if (end == CE_MORE && at != piece.size()) std::abort();
    }
    out.end = final_state(st, !partial.empty());
    return out;
}

// the reader hub's way
Out feed_items(const std::string& raw, size_t step) {
    struct Item {
        size_t off, len;
        uint8_t kind;
    };
    Out out;
    ChunkState st;
    bool in_line = false;
    std::vector<Item> items;
    std::unique_ptr<char[]> buf(new char[raw.size() ? raw.size() : 1]);
    ChunkEnd end = CE_MORE;
    for (size_t from = 0; from < raw.size() && end == CE_MORE; from += step) {
        const size_t to = std::min(raw.size(), from + step);
        std::memcpy(buf.get() + from, raw.data() + from, to - from);  // only what was "read" so far is there
        size_t at = 0;
        end = chunk_deframe(st, buf.get(), from, to, at, [&](size_t off, size_t len) {
            return split_lines(buf.get(), off, len, in_line, [&](uint8_t kind, size_t o, size_t n) {
                if (n || kind != LN_WHOLE) items.push_back(Item{o, n, kind});
                return true;
            });
        });
        if (at < from || at > to) std::abort();
    }
    std::string partial;
    for (const Item& it : items)
        join_line(partial, it.kind, buf.get() + it.off, it.len,
                  [&](const char* b, size_t bn, std::string*) { return keep(out, b, bn); });
    if (in_line != !partial.empty()) std::abort();  // the two notions of an open line are one
    out.end = end == CE_TOO_LONG || end == CE_BAD_SIZE ? "error " + chunk_error_text(st, end)
                                                       : final_state(st, in_line);
    return out;
}

std::string hex(const std::string& s) {
    static const char digits[] = "0123456789abcdef";
    std::string out;
    for (unsigned char c : s) {
        out.push_back(digits[c >> 4]);
        out.push_back(digits[c & 15]);
    }
    return out;
}

std::string unhex(const std::string& s) {
    std::string out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((char)(hexval(s[i]) * 16 + hexval(s[i + 1])));
    return out;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s FRAMINGS.tsv\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    int bad = 0;
    long feedings = 0;
    for (std::string row; std::getline(in, row);) {
        const size_t tab = row.find('\t');
        if (tab == std::string::npos) continue;
        const std::string name = row.substr(0, tab), raw = unhex(row.substr(tab + 1));
        const Out whole = feed_pieces({raw});
        auto same = [&](const Out& got, const char* how, size_t k) {
            ++feedings;
            if (got == whole) return;
            std::fprintf(stderr, "%s: %s %zu gives %zu lines, %s; whole gives %zu lines, %s\n", name.c_str(), how, k,
                         got.lines.size(), got.end.c_str(), whole.lines.size(), whole.end.c_str());
            ++bad;
        };
        for (size_t k = 1; k < raw.size(); ++k)
            same(feed_pieces({raw.substr(0, k), raw.substr(k)}), "cut at", k);
        std::vector<std::string> bytes;
        for (char c : raw) bytes.emplace_back(1, c);
        same(feed_pieces(bytes), "pieces of", 1);
        for (size_t step : {(size_t)1, (size_t)7, raw.size()}) same(feed_items(raw, step), "items in steps of", step);
        std::cout << name << '\t' << (whole.end.rfind("error ", 0) == 0 ? "error " + hex(whole.end.substr(6)) : whole.end);
        for (const std::string& line : whole.lines) std::cout << '\t' << hex(line);
        std::cout << '\n';
    }
    std::fprintf(stderr, "%ld feedings, %d disagreements\n", feedings, bad);
    return bad ? 1 : 0;
}
