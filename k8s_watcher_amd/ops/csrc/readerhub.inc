// readerhub.inc — watch sockets read on a native thread (_kwcore.ReaderHub).
// Unity-build fragment, #included into kwcore.cpp inside its anonymous
// namespace after engine.inc.
//
// On the event-loop thread the kernel's copy of every watch byte (recv) costs
// as much as splitting and applying the events it carries: at ~1M pod
// events/s (~4 GB/s of watch JSON) that is a third of the loop's time
// (profiles/loop_probe_gpu_box.md). The hub takes that copy off the loop. A
// plain-TCP watch, once its response head is parsed by asyncio, is handed to
// the hub (a dup of its socket): one thread epolls every handed-off socket,
// recv()s whatever is there into a free buffer from a fixed pool, and queues
// (stream, buffer, bytes, read time) in arrival order. It signals Python
// through an eventfd only when the queue goes from empty to non-empty, so a
// busy watch costs the loop one wake-up per batch of buffers, not one per
// socket read. Python feeds each buffer to the stream's sink (the fused
// pipeline, zero copy) and gives it back with release().
//
// Backpressure is the pool: with no free buffer the hub stops polling, the
// socket's receive queue fills and TCP flow control slows the API server —
// exactly what a paused asyncio transport does. pause(sid) does the same for
// one stream (notifier backpressure, engine/reflector.py set_paused).
//
// Read-ahead can also be bounded in bytes over all streams (max_bytes: read
// but not yet handed back; 0 = the whole pool). Many namespace watches could
// otherwise hold up to two buffers each; the budget caps that user memory.
// It is no speed-up: on the MI355X host 8-20 MiB budgets left the per-line
// cost of the namespace-watch shape where it was and starved the loop at
// times (profiles/namespace_watch_gpu_box.md).
//
// TLS: an https watch cannot be adopted mid-stream (its session lives in
// Python's ssl object), so the hub owns it from the start instead: Python
// connects the TCP socket and hands it over with a TlsContext (OpenSSL,
// built from the kubeconfig's CA / client certificate), the SNI / verified
// host name and the request bytes; the hub thread runs the handshake, writes
// the request and from then on decrypts into the same pooled buffers. The
// response head is parsed by Python from the first bytes, as on a plain
// stream, so status, headers and error bodies behave the same.

// Buffer size classes: buf_bytes, /4, /16, /64 (at least 16 KiB). A stream
// starts on the smallest and moves up one class each time a buffer fills
// before the loop takes it (a busy cluster-wide watch ends on buf_bytes: few
// large reads, one sink call each), down one when a read leaves most of its
// buffer empty — so a thousand quiet namespace watches hold small buffers and
// the pool's memory (nbufs * buf_bytes) serves them all instead of starving
// all but 64 of them.
constexpr int HUB_CLASSES = 4;

struct HubEntry {
    int sid;
    int buf;      // -1: end of stream (err: 0 = orderly close, else errno)
    size_t len;
    int64_t read_ns;
    int err;
};

// Hub-side framing of a chunked watch body bound to a native Pipeline
// (start_framing): the thread that just recv()d the bytes — still in its
// cache — runs the HTTP chunk de-framing and NDJSON line splitting
// (chunked.inc) that the pipeline's pl_more / pl_segment (engine.inc) would
// run on the event-loop thread, and leaves per buffer a list of line items.
// The loop then only walks the items: its split stage was 60-70 ns per line
// on the cluster watch and 140-150 with many namespace watches, whose
// buffers wait longer and go cold (profiles/namespace_watch_r3_gpu_box.md).
// A stream's chunked-body state: the pipeline's ChunkState, taken over as it
// is, plus whether a line is open (the pipeline's partial is not empty).
struct HubFramer {
    bool on = false;
    bool stopped = false;  // end of body or a framing error: later bytes are not framed
    bool in_line = false;
    ChunkState chunk;

    // frame bytes [from, to) of the buffer `base` into f (f.upto == from)
    void frame(const char* base, size_t from, size_t to, HubFrame& f) {
        f.upto = to;
        if (stopped) return;
        auto item = [&f](uint8_t kind, size_t off, size_t len) {
            if (len || kind != HI_LINE) f.items.push_back(HubItem{(uint32_t)off, (uint32_t)len, kind});
            return true;
        };
        size_t at;
        const ChunkEnd end = chunk_deframe(chunk, base, from, to, at, [&](size_t off, size_t len) {
            return split_lines(base, off, len, in_line, item);
        });
        if (end == CE_MORE) return;
        stopped = true;
        if (end != CE_DONE) f.error = chunk_error_text(chunk, end);
        item(end == CE_DONE ? HI_DONE : HI_ERROR, at, 0);
    }
};

struct HubStream {
    int fd = -1;
    bool paused = false;
    uint32_t armed = 0;  // events registered with epoll
    int open = -1;       // index in ready_ of this stream's newest entry while it has room
    int held = 0;        // buffers of this stream queued or still held by Python
    bool reading = false;  // the thread is in recv on it, outside the lock (read_one)
    bool removed = false;  // remove() came meanwhile: the thread drops it when it is back
    SSL* ssl = nullptr;  // TLS streams (add_tls)
    int phase = 0;       // 0 streaming, 1 TLS handshake, 2 writing the request
    bool want_out = false;  // EPOLLOUT: handshake / request / TLS record layer wants to write
    bool starved = false;   // disarmed because the pool or byte budget ran out (in starved_)
    int cls = HUB_CLASSES - 1;  // buffer size class of its next read (0: the largest)
    int reading_buf = -1;  // the buffer read_one is filling while `reading`
    HubFramer framer;      // start_framing: this stream's bytes are framed by the hub
    TlsSecrets* secrets = nullptr;  // TLS: the traffic secrets OpenSSL reports (keylog callback)
    // TLS 1.3 + AES-GCM after the request: the hub reads and opens the
    // records itself (tls13.inc), on the CryptoPool — SSL_read no more
    std::unique_ptr<Tls13Rx> rx;
    size_t ring_counted = 0;  // rx's ciphertext memory as counted in ring_bytes_ (mu_)
    std::string out;     // the request, until written
    size_t out_off = 0;
    int64_t last_ns = 0;  // (mu_) when its last read with bytes ended (CLOCK_MONOTONIC)
    int reader = -1;      // the reader thread that polls it (ReaderHub::readers_)
    // (mu_) since when the hub has not been polling it for reads although it
    // is streaming and not paused (CLOCK_MONOTONIC; 0: polled, paused, setting
    // up or ended). Written by arm() / strand() when that changes, never per
    // read: what the stall guard's tick goes by (ReaderHub::stall_tick)
    int64_t off_since_ns = 0;
};

// _kwcore.TlsContext: an OpenSSL client context for watch streams.
struct TlsCtxObject {
    PyObject_HEAD
    SSL_CTX* ctx;
    int verify;
};

// Read-ahead per stream: at most this many buffers queued or in use (the
// default; set_depth). A stream at the limit is not polled until Python
// releases one, so a slow loop leaves the backlog in the socket (TCP flow
// control) rather than in user memory.
constexpr int HUB_MAX_HELD = 2;
constexpr int HUB_MAX_READERS = 8;
constexpr int64_t HUB_RING_SHRINK_NS = 1000000000LL;  // a TLS ring larger than its stream needs this long shrinks
constexpr int HUB_MAX_DEPTH = 8;
// Starved streams re-armed per buffer handed back (give_back).
constexpr int HUB_STARVED_WAKE = 2;
// The stall guard's tick: a quarter of the guard, at most this (set_stall_guard).
constexpr int64_t HUB_STALL_TICK_NS = 250000000LL;

// last_stall(): the stream the stall guard re-armed last
struct HubStall {
    int sid = 0;  // 0: none yet
    int64_t age_ns = 0;  // how long it had been off, with bytes waiting
    std::vector<long long> state;  // its stream_state just before the re-arm
};



class ReaderHub {
    // a reader thread: its epoll set, its wake-up eventfd (readers_ below)
    struct Reader {
        int ep = -1, wake_fd = -1;
        int streams = 0;  // (mu_) streams given to it
        std::thread th;
        std::atomic<int> tid{0};
        std::atomic<int64_t> oldest_ns{0};  // the stall guard's figure over this thread's streams (stall_tick)
        int64_t next_tick_ns = 0;           // (its own thread) when its next tick is due
    };

  public:
    ReaderHub(size_t buf_bytes, int nbufs, size_t max_bytes = 0)
        : buf_bytes_(buf_bytes), pool_bytes_((size_t)nbufs * buf_bytes),
          max_bytes_(max_bytes ? max_bytes : (size_t)nbufs * buf_bytes) {
        // allocated on first use, reused last-in first-out per size class: a
        // busy cluster-wide watch keeps cycling the same few buffers (the
        // resident set stays small) while many quiet namespace watches each
        // hold a small one
        const size_t ids = std::max<size_t>((size_t)nbufs, std::min<size_t>(8192, pool_bytes_ / class_bytes(HUB_CLASSES - 1)));
        bufs_.resize(ids);
        frames_.resize(ids);
        cap_.assign(ids, 0);
        cls_.assign(ids, 0);
        owner_.assign(ids, 0);
        buf_len_.assign(ids, 0);
        for (size_t i = ids; i-- > 0;) spare_.push_back((int)i);
        py_fd_ = eventfd(0, EFD_NONBLOCK | EFD_CLOEXEC);
        start_reader();
    }
    ~ReaderHub() { stop(); }

    bool ok() const { return !readers_.empty() && readers_[0]->ep >= 0 && readers_[0]->wake_fd >= 0 && py_fd_ >= 0; }
    int py_fd() const { return py_fd_; }

    // n reader threads in all (1..HUB_MAX_READERS); before streams are added
    // (streams added later are spread over them: the one with fewest first)
    bool set_readers(int n) {
        std::lock_guard<std::mutex> g(mu_);
        if (n < 1 || n > HUB_MAX_READERS || (int)readers_.size() > n) return (int)readers_.size() == n;
        while ((int)readers_.size() < n)
            if (!start_reader()) return false;
        return true;
    }
    int readers() {
        std::lock_guard<std::mutex> g(mu_);
        return (int)readers_.size();
    }

    void stop() {
        quit_.store(true);
        wake();
        for (auto& r : readers_)
            if (r->th.joinable()) r->th.join();
        std::lock_guard<std::mutex> g(mu_);
        for (auto& kv : streams_) release_stream(kv.second);
        streams_.clear();
        for (auto& r : readers_)
            for (int* fd : {&r->ep, &r->wake_fd})
                if (*fd >= 0) {
                    ::close(*fd);
                    *fd = -1;
                }
        if (py_fd_ >= 0) {
            ::close(py_fd_);
            py_fd_ = -1;
        }
    }

    // takes ownership of fd (a dup of the watch socket); returns the stream id
    int add(int fd) {
        std::lock_guard<std::mutex> g(mu_);
        const int sid = next_sid_++;
        HubStream& s = streams_[sid];
        s.fd = fd;
        give_reader(s);
        arm(sid, s);
        return sid;
    }

    // a TLS stream (fd: a connected socket, owned from here on): handshake,
    // then `request` is written, then the decrypted response is read like any
    // other stream. Returns the stream id.
    int add_tls(int fd, SSL_CTX* ctx, bool verify, const std::string& host, std::string&& request,
                std::string& error) {
        std::lock_guard<std::mutex> g(mu_);
        SSL* ssl = SSL_new(ctx);
        if (!ssl || SSL_set_fd(ssl, fd) != 1) {
            error = tls_error("setup failed");
            if (ssl) SSL_free(ssl);
            return -1;
        }
        unsigned char ipbuf[16];
        const bool is_ip = inet_pton(AF_INET, host.c_str(), ipbuf) == 1 || inet_pton(AF_INET6, host.c_str(), ipbuf) == 1;
        if (!is_ip && !host.empty()) SSL_set_tlsext_host_name(ssl, host.c_str());
        if (verify && !host.empty()) {
            const int ok = is_ip ? X509_VERIFY_PARAM_set1_ip_asc(SSL_get0_param(ssl), host.c_str())
                                 : SSL_set1_host(ssl, host.c_str());
            if (ok != 1) {
                error = tls_error("host name setup failed");
                SSL_free(ssl);
                return -1;
            }
        }
        SSL_set_connect_state(ssl);
        const int sid = next_sid_++;
        HubStream& s = streams_[sid];
        s.fd = fd;
        give_reader(s);
        s.ssl = ssl;
        s.secrets = new TlsSecrets();
        SSL_set_ex_data(ssl, g_tls_ex, s.secrets);
        s.phase = 1;
        s.want_out = true;  // writable at once: the thread sends the ClientHello
        s.out = std::move(request);
        arm(sid, s);
        return sid;
    }

    // why a stream ended with err < 0 (TLS failures), once
    std::string error_text(int sid) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = errors_.find(sid);
        if (it == errors_.end()) return std::string();
        std::string e = std::move(it->second);
        errors_.erase(it);
        return e;
    }

    // forget a stream: its socket is closed here, its queued buffers freed
    void remove(int sid) {
        std::lock_guard<std::mutex> g(mu_);
        errors_.erase(sid);
        tls_pending_.erase(sid);
        auto it = streams_.find(sid);
        int busy = -1;  // the open entry the thread is appending to right now: it drops that one
        if (it != streams_.end()) {
            if (it->second.reading) {
                // the thread is inside recv on this socket: it closes the stream
                // (and drops the buffer it is filling) when it comes back
                it->second.removed = true;
                busy = it->second.open;
            } else {
                if (it->second.fd >= 0) epoll_ctl(ep_of(it->second), EPOLL_CTL_DEL, it->second.fd, nullptr);
                release_stream(it->second);
                drop_from_reader(it->second);
                streams_.erase(it);
            }
        }
        bool queued = false;  // nothing of this stream waiting (the usual case): ready_ stays as is
        for (size_t i = 0; i < ready_.size() && !queued; ++i) queued = ready_[i].sid == sid && (int)i != busy;
        if (!queued) return;
        std::vector<HubEntry> keep;
        for (size_t i = 0; i < ready_.size(); ++i) {
            const HubEntry& e = ready_[i];
            if (e.sid == sid && (int)i != busy) {
                if (e.buf >= 0) give_back(e.buf);
            } else {
                keep.push_back(e);
            }
        }
        ready_.swap(keep);
        reopen();
    }

    // (mu_ held) after ready_ was compacted: each stream's newest queued entry
    // with room is open for appends again
    void reopen() {
        for (auto& kv : streams_) {
            kv.second.open = -1;
            for (int i = (int)ready_.size() - 1; i >= 0; --i)
                if (ready_[(size_t)i].sid == kv.first) {
                    if (ready_[(size_t)i].buf >= 0 && ready_[(size_t)i].len < cap_[(size_t)ready_[(size_t)i].buf])
                        kv.second.open = i;
                    break;
                }
        }
    }

    void pause(int sid, bool paused) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = streams_.find(sid);
        if (it == streams_.end()) return;
        it->second.paused = paused;
        arm(sid, it->second);
    }

    std::vector<HubEntry> take() {
        uint64_t v;
        ssize_t r = ::read(py_fd_, &v, 8);  // clear the signal before looking
        (void)r;
        std::lock_guard<std::mutex> g(mu_);
        std::vector<HubEntry> out, keep;
        for (size_t i = 0; i < ready_.size(); ++i) {
            // an entry the thread is appending to (outside the lock) stays
            // queued: it is that stream's newest, so per-stream order holds,
            // and the thread signals again once it is done with it
            auto it = streams_.find(ready_[i].sid);
            if (it != streams_.end() && it->second.reading && it->second.open == (int)i) {
                keep.push_back(ready_[i]);
                continue;
            }
            out.push_back(ready_[i]);
        }
        ready_.swap(keep);
        for (auto& kv : streams_) kv.second.open = -1;  // taken entries are closed to appends
        for (size_t i = 0; i < ready_.size(); ++i) {
            streams_[ready_[i].sid].open = (int)i;
            deferred_ = true;
        }
        return out;
    }

    const char* buf(int i) const { return bufs_[(size_t)i].get(); }

    void release(int i) {
        std::lock_guard<std::mutex> g(mu_);
        give_back(i);
    }

    // kernel thread id of reader thread i (0: the first), 0 if none
    int tid(int i = 0) const {
        if (i < 0 || (size_t)i >= readers_.size()) return 0;
        int t = 0;
        for (int spin = 0; spin < 2000 && !(t = readers_[(size_t)i]->tid.load()); ++spin) usleep(50);
        return t;
    }
    long long reads() const { return reads_.load(); }
    long long over_budget() const { return over_budget_.load(); }
    size_t max_bytes() const { return max_bytes_; }
    long long wakeups() const { return signals_.load(); }
    long long starved() const { return starved_.load(); }
    long long framed_reads() const { return framed_reads_.load(); }
    long long recv_ns() const { return recv_ns_.load(); }
    long long frame_ns() const { return frame_ns_.load(); }
    long long recv_bytes() const { return recv_bytes_.load(); }
    long long idle_ns() const { return idle_ns_.load(); }
    long long held_waits() const { return held_waits_.load(); }
    // when stream sid's last read with bytes ended (CLOCK_MONOTONIC ns), 0 if none / unknown
    int64_t last_read(int sid) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = streams_.find(sid);
        return it == streams_.end() ? 0 : it->second.last_ns;
    }
    // a stream's polling state, for diagnosing a stalled stream: (armed epoll
    // events, buffers held, open entry, reading, starved, paused, size class,
    // reader thread, fd, queued entries); empty if unknown
    // ... then the hub's bytes held, its byte budget, the length of the
    // starved queue and how often this stream is in it
    std::vector<long long> stream_state(int sid) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = streams_.find(sid);
        if (it == streams_.end()) return {};
        return state_of(sid, it->second);
    }

    // The stall guard. A stream the hub is not polling must be one that
    // give_back() (or a resume) will poll again; a wake-up lost in arm() /
    // give_back() leaves one that nothing re-arms, its bytes unread until the
    // reflector's idle limit reconnects it minutes later. With the guard on
    // (seconds > 0; 0 = off: the threads sleep in epoll_wait without a
    // timeout, as without it) each reader thread looks at its streams at most
    // once per tick = min(250 ms, seconds / 4), reports how long bytes have
    // been waiting on a stream it is not polling (oldest_unread_ns) and
    // re-arms one that waited `seconds` (stall_tick).
    void set_stall_guard(double seconds) {
        int64_t ns = seconds > 0 ? (int64_t)(seconds * 1e9) : 0;
        if (seconds > 0 && ns < 4000000) ns = 4000000;  // a tick of a millisecond at least
        stall_ns_.store(ns);
        std::lock_guard<std::mutex> g(mu_);
        wake();  // a thread asleep without a timeout takes the new setting up
    }
    int64_t stall_guard_ns() const { return stall_ns_.load(); }
    // The largest figure over the reader threads, 0 with none: an upper bound
    // on the age of the oldest unread byte — the time since polling of a
    // stream stopped, counted only while bytes wait on it (they may have
    // arrived any time since). As of the threads' last ticks.
    int64_t oldest_unread_ns() {
        std::lock_guard<std::mutex> g(mu_);
        int64_t a = 0;
        for (auto& r : readers_) a = std::max(a, r->oldest_ns.load(std::memory_order_relaxed));
        return a;
    }
    long long stall_recoveries() const { return stall_recoveries_.load(); }
    HubStall last_stall() {
        std::lock_guard<std::mutex> g(mu_);
        return last_stall_;
    }
    // Diagnostics hook (tests of the stall guard): leave stream sid as a lost
    // wake-up would — EPOLLIN off, not in the starved queue, so nothing but
    // the guard re-arms it. For a stream at rest (no read of it under way).
    bool strand(int sid) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = streams_.find(sid);
        if (it == streams_.end() || it->second.fd < 0) return false;
        HubStream& s = it->second;
        const uint32_t want = s.armed & ~(uint32_t)(EPOLLIN | EPOLLRDHUP);
        epoll_event ev{};
        ev.events = want;
        ev.data.u32 = (uint32_t)sid;
        epoll_ctl(ep_of(s), EPOLL_CTL_MOD, s.fd, &ev);
        s.armed = want;
        if (!s.phase && !s.paused && !s.off_since_ns) s.off_since_ns = mono_ns();
        return true;
    }
    long long ring_resizes() {
        std::lock_guard<std::mutex> g(mu_);
        return ring_resizes_;
    }
    // TLS record layer: take over TLS 1.3 streams (records) and open their
    // records on `threads` pool threads besides the reader (0: the reader
    // alone). Before any stream is added.
    void set_tls(bool records, int threads) {
        std::lock_guard<std::mutex> g(mu_);
        tls_records_ = records;
        pool_.reset(records && threads > 0 ? new CryptoPool(threads) : nullptr);
    }
    long long tls_taken() const { return tls_taken_.load(); }
    long long tls_kept() const { return tls_kept_.load(); }
    long long tls_ct_bytes() const { return tls_ct_bytes_.load(); }
    long long decrypt_ns() const { return decrypt_ns_.load(); }
    long long tls_pool_wait_ns() const { return pool_ ? pool_->wait_ns() : 0; }
    std::vector<int> tls_thread_ids() {
        std::lock_guard<std::mutex> g(mu_);
        return pool_ ? pool_->thread_ids() : std::vector<int>();
    }
    std::vector<std::pair<long long, long long>> tls_pool() const {
        return pool_ ? pool_->stats() : std::vector<std::pair<long long, long long>>();
    }
    // records opened, of them on the pool, key updates, session tickets (all streams)
    std::array<long long, 4> tls_records() {
        std::lock_guard<std::mutex> g(mu_);
        std::array<long long, 4> a = tls_done_;
        for (auto& kv : streams_)
            if (kv.second.rx) {
                a[0] += kv.second.rx->records;
                a[1] += kv.second.rx->pooled;
                a[2] += kv.second.rx->key_updates;
                a[3] += kv.second.rx->tickets;
            }
        return a;
    }
    void set_depth(int n) {
        std::lock_guard<std::mutex> g(mu_);
        max_held_ = n;
        wake();  // streams waiting at the old limit may read now
    }
    int depth() {
        std::lock_guard<std::mutex> g(mu_);
        return max_held_;
    }
    // memory accounting: read buffers and TLS ciphertext rings allocated so
    // far (both within the pool's memory), bytes queued or held by Python, and
    // of the first the rings alone
    std::array<size_t, 3> memory() {
        std::lock_guard<std::mutex> g(mu_);
        return {alloc_bytes_ + ring_bytes_, held_bytes_, ring_bytes_};
    }

  private:
    // (mu_ held, or the constructor) one more reader thread with its own epoll set
    bool start_reader() {
        std::unique_ptr<Reader> r(new Reader());
        r->ep = epoll_create1(EPOLL_CLOEXEC);
        r->wake_fd = eventfd(0, EFD_NONBLOCK | EFD_CLOEXEC);
        if (r->ep < 0 || r->wake_fd < 0) {
            if (r->ep >= 0) ::close(r->ep);
            if (r->wake_fd >= 0) ::close(r->wake_fd);
            return false;
        }
        epoll_event ev{};
        ev.events = EPOLLIN;
        ev.data.u32 = UINT32_MAX;
        epoll_ctl(r->ep, EPOLL_CTL_ADD, r->wake_fd, &ev);
        Reader* rp = r.get();
        readers_.push_back(std::move(r));
        rp->th = std::thread([this, rp] {
            rp->tid.store((int)syscall(SYS_gettid));
            loop(*rp);
        });
        return true;
    }

    // (mu_ held) a new stream goes to the reader thread with the fewest
    void give_reader(HubStream& s) {
        int best = 0;
        for (int i = 1; i < (int)readers_.size(); ++i)
            if (readers_[(size_t)i]->streams < readers_[(size_t)best]->streams) best = i;
        s.reader = best;
        ++readers_[(size_t)best]->streams;
    }
    // (mu_ held) a stream leaves its reader thread for good
    void drop_from_reader(HubStream& s) {
        if (s.reader >= 0 && (size_t)s.reader < readers_.size()) --readers_[(size_t)s.reader]->streams;
        s.reader = -1;
    }
    int ep_of(const HubStream& s) const {
        return s.reader >= 0 && (size_t)s.reader < readers_.size() ? readers_[(size_t)s.reader]->ep : -1;
    }

    void wake() {
        uint64_t one = 1;
        for (auto& r : readers_) {
            ssize_t k = ::write(r->wake_fd, &one, 8);
            (void)k;
        }
    }

    // (mu_ held) EPOLLIN on unless paused, ended or the pool is empty;
    // EPOLLOUT while the handshake, the request or a TLS record wants to write
    void arm(int sid, HubStream& s) {
        if (s.fd < 0) return;
        const bool pool = s.open >= 0 || can_acquire(s.cls, s.held == 0);
        const bool in = s.phase ? true
                                : !s.paused && held_bytes_ < max_bytes_ && pool &&
                                      (s.held < max_held_ || s.open >= 0);
        if (!in && !s.paused && !s.starved && (held_bytes_ >= max_bytes_ || !pool)) {
            s.starved = true;  // give_back re-arms exactly these (starved_sids_), not every stream
            starved_sids_.push_back(sid);
        }
        // the stall guard's clock: runs from the moment a streaming, unpaused
        // stream is left unpolled, stops when it is polled again or paused
        if (in || s.paused)
            s.off_since_ns = 0;
        else if (!s.off_since_ns)
            s.off_since_ns = mono_ns();
        const uint32_t want = (in ? (EPOLLIN | EPOLLRDHUP) : 0) | (s.want_out ? EPOLLOUT : 0);
        if (want == s.armed) return;
        epoll_event ev{};
        ev.events = want;
        ev.data.u32 = (uint32_t)sid;
        const int ep = ep_of(s);
        if (epoll_ctl(ep, EPOLL_CTL_MOD, s.fd, &ev) < 0 && errno == ENOENT) epoll_ctl(ep, EPOLL_CTL_ADD, s.fd, &ev);
        s.armed = want;
    }

    // (mu_ held)
    void release_stream(HubStream& s) {
        if (s.rx) {
            ring_bytes_ -= std::min(ring_bytes_, s.ring_counted);
            s.ring_counted = 0;
            --rx_streams_;
            tls_done_[0] += s.rx->records;
            tls_done_[1] += s.rx->pooled;
            tls_done_[2] += s.rx->key_updates;
            tls_done_[3] += s.rx->tickets;
        }
        if (s.ssl) {
            SSL_free(s.ssl);
            s.ssl = nullptr;
        }
        delete s.secrets;  // (wipes)
        s.secrets = nullptr;
        s.rx.reset();  // (its Tls13Dir wipes the traffic secret and keys)
        if (s.fd >= 0) {
            ::close(s.fd);
            s.fd = -1;
        }
    }

    // (mu_ held) end a stream: no more polling; Python sees an end entry
    void finish(int sid, HubStream& s, int err, const std::string& why = std::string()) {
        if (s.fd >= 0) epoll_ctl(ep_of(s), EPOLL_CTL_DEL, s.fd, nullptr);
        s.armed = 0;
        s.off_since_ns = 0;
        release_stream(s);
        s.open = -1;
        tls_pending_.erase(sid);
        if (!why.empty()) errors_[sid] = why;
        push(HubEntry{sid, -1, 0, mono_ns(), err});
    }

    // (mu_ held) TLS handshake, then the request; on to streaming when done
    void drive_setup(int sid, HubStream& s) {
        if (s.phase == 1) {
            ERR_clear_error();
            const int r = SSL_do_handshake(s.ssl);
            if (r != 1) {
                const int e = SSL_get_error(s.ssl, r);
                if (e == SSL_ERROR_WANT_READ || e == SSL_ERROR_WANT_WRITE) {
                    s.want_out = e == SSL_ERROR_WANT_WRITE;
                    arm(sid, s);
                    return;
                }
                std::string why = tls_error("handshake with the API server failed");
                const long v = SSL_get_verify_result(s.ssl);
                if (v != X509_V_OK) why += std::string(" (") + X509_verify_cert_error_string(v) + ")";
                finish(sid, s, -1, why);
                return;
            }
            s.phase = 2;
        }
        while (s.out_off < s.out.size()) {
            ERR_clear_error();
            const int k = SSL_write(s.ssl, s.out.data() + s.out_off, (int)(s.out.size() - s.out_off));
            if (k > 0) {
                s.out_off += (size_t)k;
                continue;
            }
            const int e = SSL_get_error(s.ssl, k);
            if (e == SSL_ERROR_WANT_READ || e == SSL_ERROR_WANT_WRITE) {
                s.want_out = e == SSL_ERROR_WANT_WRITE;
                arm(sid, s);
                return;
            }
            finish(sid, s, -1, tls_error("writing the watch request failed"));
            return;
        }
        std::string().swap(s.out);
        s.phase = 0;
        s.want_out = false;
        if (tls_records_) take_records(s);
        arm(sid, s);
        if (!s.paused && held_bytes_ < max_bytes_ && (s.open >= 0 || (can_acquire(s.cls, s.held == 0) && s.held < max_held_)))
            read_one(sid, s);  // the response may have arrived with the handshake's last flight
    }

    // (mu_ held) the request is out: from here on the hub opens this stream's
    // records itself if the session allows (TLS 1.3, AES-GCM, secret seen,
    // nothing buffered inside OpenSSL) — else SSL_read stays
    void take_records(HubStream& s) {
        Tls13Dir d;
        const bool take = SSL_pending(s.ssl) == 0 && !SSL_has_pending(s.ssl) && tls13_server_dir(s.ssl, s.secrets, d);
        s.secrets->wipe();  // copied into d, or not wanted: no copy of the secret stays behind
        if (!take) {
            ++tls_kept_;
            return;
        }
        s.rx.reset(new Tls13Rx());
        s.rx->d = d;
        s.rx->wrap.reserve(5 + TLS_CT_MAX);  // (fixed: counted once)
        ++rx_streams_;
        ++tls_taken_;
        count_ring(s);
    }

    // (mu_ held) a record-layer stream's ring for reads into buffers of `cap`
    // bytes: this batch and the next one the reader receives while the pool
    // opens it. Sized under the lock before each read — grown when the
    // stream's class grows, shrunk when it drops (a quiet stream goes back to
    // a small ring) — and counted in the pool's memory (ring_bytes_).
    // While the rings would pass the pool's memory, a stream's ring is the
    // smallest that still moves (two records).
    static size_t ring_for(size_t cap) { return 2 * (cap + (cap >> 9) + TLS_CT_MAX + 5); }
    // A ring grows at once; it shrinks only after it has been larger than
    // its stream needs for HUB_RING_SHRINK_NS: a busy stream's buffer class
    // moves up and down between reads, and a resize per read (a multi-MiB
    // allocation and copy under the lock) had cut one https stream from
    // 1.35M to 0.76M ev/s.
    void size_ring(HubStream& s, size_t cap) {
        Tls13Rx& rx = *s.rx;
        size_t want = ring_for(cap);
        if (ring_bytes_ - std::min(ring_bytes_, s.ring_counted) + want > pool_bytes_) want = ring_for(0);
        const size_t have = rx.ct.size();
        if (have < want) {
            if (rx.resize(want)) ++ring_resizes_;
            rx.big_since_ns = 0;
        } else if (have > want) {
            const int64_t now = mono_ns();
            if (!rx.big_since_ns) rx.big_since_ns = now;
            // (a stream squeezed by the pool's memory shrinks at once)
            const bool squeezed = want == ring_for(0) && ring_bytes_ > pool_bytes_ / 2;
            if ((squeezed || now - rx.big_since_ns >= HUB_RING_SHRINK_NS) && rx.pending() <= want && rx.resize(want)) {
                ++ring_resizes_;
                rx.big_since_ns = 0;
            }
        } else {
            rx.big_since_ns = 0;
        }
        count_ring(s);
    }
    // (mu_ held) bring ring_bytes_ up to date with the stream's ring memory
    void count_ring(HubStream& s) {
        const size_t now = s.rx ? s.rx->ring_bytes() : 0;
        ring_bytes_ = ring_bytes_ - std::min(ring_bytes_, s.ring_counted) + now;
        s.ring_counted = now;
    }

    // A record-layer stream's read (unlocked, like stream_read): ciphertext
    // into rx.ct, whole records opened into p[len, cap). Sets err (0 closed,
    // 1 failed, -1 open), why, t (first byte's time), got (plaintext bytes).
    // While the pool opens one batch, this thread receives the next one
    // (rx.ct holds two batches' worth), so recv and decryption overlap.
    void rx_read(HubStream& s, char* p, size_t& len, size_t cap, size_t budget, size_t& got, int64_t& t, int& err,
                 std::string& why, bool& over, int64_t& rc_ns, int64_t& dec_ns) {
        Tls13Rx& rx = *s.rx;
        bool drained = false;
        // receive into the ring until `upto` bytes are pending (or it is full)
        auto receive = [&](size_t upto) {
            const int64_t r0 = mono_ns();
            const size_t c = rx.ct.size();
            upto = std::min(upto, c);
            while (!rx.eof && err <= 0 && rx.pending() < upto) {
                const size_t at = (size_t)(rx.tail % c);
                const size_t n = std::min(c - at, upto - rx.pending());
                const ssize_t k = ::recv(s.fd, rx.ct.data() + at, n, MSG_DONTWAIT);
                if (k > 0) {
                    const int64_t now = mono_ns();
                    if (!t) t = now;
                    if (!rx.since_ns) rx.since_ns = now;  // the oldest unopened byte's arrival
                    rx.last_ns = now;
                    rx.tail += (size_t)k;
                    tls_ct_bytes_.fetch_add(k, std::memory_order_relaxed);
                    reads_.fetch_add(1, std::memory_order_relaxed);
                    continue;
                }
                if (k == 0) {
                    rx.eof = true;
                    break;
                }
                if (errno == EINTR) continue;
                if (errno == EAGAIN || errno == EWOULDBLOCK) {
                    drained = true;
                    break;
                }
                why = std::strerror(errno);
                err = 1;
                break;
            }
            rc_ns += mono_ns() - r0;
        };
        for (;;) {
            const size_t room = cap - len;
            const size_t want_ct = room + (room >> 9) + TLS_CT_MAX + 5;  // (the ring holds two: size_ring)
            drained = false;
            receive(want_ct);
            if (err > 0) return;
            const int64_t d0 = mono_ns();
            int64_t overlap = 0;
            const long long w = tls13_rx_open(rx, reinterpret_cast<uint8_t*>(p + len), room, pool_.get(), recs_, [&] {
                const int64_t o0 = mono_ns();
                receive(2 * want_ct);  // the next batch's records, while the pool opens this one
                overlap += mono_ns() - o0;
            });
            dec_ns += mono_ns() - d0 - overlap;
            // the batch's bytes may have been received by an earlier read (the
            // overlap): its read time is when they arrived, never 0
            if (w > 0 && (!t || (rx.since_ns && rx.since_ns < t))) t = rx.since_ns ? rx.since_ns : mono_ns();
            rx.since_ns = rx.pending() ? rx.last_ns : 0;
            if (w < 0) {
                why = rx.error;
                err = 1;
                return;
            }
            len += (size_t)w;
            got += (size_t)w;
            if (rx.failed) {  // what came before the bad record is in; the stream ends with the error
                why = rx.error;
                err = 1;
                return;
            }
            if (err > 0) return;
            if (rx.closed || (rx.eof && !rx.whole_record())) {  // the server ended the stream
                err = 0;
                if (!rx.closed && rx.pending()) {  // mid-record: truncated, not a close
                    why = "TLS: the watch stream was truncated inside a record";
                    err = 1;
                }
                return;
            }
            if (got >= budget) {
                over = true;
                return;
            }
            if ((drained && !rx.whole_record()) || len >= cap || w == 0) return;
        }
    }

    // >0 bytes; 0 = closed by the peer; -1 = would block; -2 = failed (why set).
    // Runs without the lock: touches only the socket / TLS session, and
    // reports a TLS write wish through `want_write` (s.want_out is the lock's).
    ssize_t stream_read(const HubStream& s, char* p, size_t n, std::string& why, bool& want_write) {
        if (!s.ssl) {
            while (true) {
                ssize_t k = ::recv(s.fd, p, n, MSG_DONTWAIT);
                if (k >= 0) return k;
                if (errno == EINTR) continue;
                if (errno == EAGAIN || errno == EWOULDBLOCK) return -1;
                why = std::strerror(errno);
                return -2;
            }
        }
        ERR_clear_error();
        const int k = SSL_read(s.ssl, p, (int)std::min<size_t>(n, 1u << 30));
        if (k > 0) return k;
        const int e = SSL_get_error(s.ssl, k);
        if (e == SSL_ERROR_WANT_READ) return -1;
        if (e == SSL_ERROR_WANT_WRITE) {  // a TLS record to send first (key update)
            want_write = true;
            return -1;
        }
        if (e == SSL_ERROR_ZERO_RETURN) return 0;
        if (e == SSL_ERROR_SYSCALL && ERR_peek_error() == 0) return 0;  // closed without close_notify
        why = tls_error("reading the watch stream failed");
        return -2;
    }

    size_t class_bytes(int c) const {
        return std::max<size_t>(buf_bytes_ >> (2 * c), std::min<size_t>(buf_bytes_, 16384));
    }

    // (mu_ held) the largest class a stream may grow to: one buffer of it per
    // stream fits the pool. Growing past its share, every busy stream of a
    // thousand namespace watches climbed to buf_bytes and all but 64 starved
    // (profiles/namespace_watch_r3_gpu_box.md); each starved stream then cost
    // the loop's release() an epoll re-arm.
    // A record-layer (TLS) stream also holds a ring of about twice its
    // buffer class, so it counts three times.
    int fair_cls() const {
        const size_t n = std::max<size_t>(1, streams_.size() + 2 * rx_streams_);
        for (int c = 0; c < HUB_CLASSES - 1; ++c)
            if (class_bytes(c) * n <= pool_bytes_) return c;
        return HUB_CLASSES - 1;
    }

    // (mu_ held) could a buffer of class c be had now (free, or allocated
    // within the pool's memory, dropping free buffers of other classes)? The
    // pool's memory holds the TLS rings too — but a stream's first buffer
    // only has to fit beside the other buffers: no stream starves behind
    // rings (a ring is only sized once its stream has a buffer).
    bool can_acquire(int c, bool first = false) const {
        if (!free_[c].empty()) return true;
        size_t droppable = 0;
        bool any_free = false;
        for (int k = 0; k < HUB_CLASSES; ++k)
            if (k != c) {
                droppable += free_[k].size() * class_bytes(k);
                any_free |= !free_[k].empty();
            }
        const size_t rings = first ? 0 : ring_bytes_;
        return alloc_bytes_ + rings - droppable + class_bytes(c) <= pool_bytes_ && (!spare_.empty() || any_free);
    }

    // (mu_ held) a buffer of class c, or -1
    int acquire(int c, bool first = false) {
        if (!free_[c].empty()) {
            const int b = free_[c].back();
            free_[c].pop_back();
            return b;
        }
        const size_t need = class_bytes(c);
        // make room: free buffers of other classes go, the largest first
        const size_t used = first ? 0 : ring_bytes_;  // TLS rings share the pool's memory (can_acquire)
        for (int k = 0; k < HUB_CLASSES && (alloc_bytes_ + used + need > pool_bytes_ || spare_.empty()); ++k)
            while (k != c && !free_[k].empty() && (alloc_bytes_ + used + need > pool_bytes_ || spare_.empty())) {
                const int b = free_[k].back();
                free_[k].pop_back();
                drop(b);
            }
        if (alloc_bytes_ + used + need > pool_bytes_ || spare_.empty()) return -1;
        const int b = spare_.back();
        bufs_[(size_t)b].reset(new (std::nothrow) char[need]);
        if (!bufs_[(size_t)b]) return -1;
        spare_.pop_back();
        cap_[(size_t)b] = need;
        cls_[(size_t)b] = c;
        alloc_bytes_ += need;
        return b;
    }

    // (mu_ held) give a free buffer's memory back
    void drop(int b) {
        alloc_bytes_ -= cap_[(size_t)b];
        bufs_[(size_t)b].reset();
        cap_[(size_t)b] = 0;
        spare_.push_back(b);
    }

    // (mu_ held) bytes are waiting for a read of s (or it is being read, or
    // its TLS layer holds some): re-arming it will lead to a read
    static bool has_bytes(const HubStream& s) {
        if (s.reading || s.fd < 0) return true;
        if (s.rx && (s.rx->whole_record() || s.rx->eof)) return true;
        if (s.ssl && SSL_pending(s.ssl) > 0) return true;
        int n = 0;
        return ioctl(s.fd, FIONREAD, &n) != 0 || n > 0;
    }

    // (mu_ held) stream_state()
    std::vector<long long> state_of(int sid, const HubStream& st) const {
        long long queued = 0, in_starved = 0;
        for (const HubEntry& e : ready_) queued += e.sid == sid;
        for (int x : starved_sids_) in_starved += x == sid;
        return {(long long)st.armed, st.held, st.open, st.reading, st.starved, st.paused, st.cls, st.reader, st.fd, queued,
                (long long)held_bytes_, (long long)max_bytes_, (long long)starved_sids_.size(), in_starved};
    }

    // (mu_ held, reader thread `me`) the stall guard's tick over this
    // thread's streams. Only a stream that has been off for longer than a
    // tick is probed (has_bytes: an ioctl) — at saturation streams go off and
    // on again within milliseconds and none is. A stream off that long with
    // bytes waiting counts with the time since it went off: an upper bound on
    // its bytes' age. One that reaches the guard is re-armed; it counts as
    // recovered only if that turned EPOLLIN on. A stream arm() leaves off is
    // short of pool or byte budget, or at its read-ahead limit because the
    // loop has not released a buffer: not a stall of the hub's, and its age
    // goes on growing (the readiness check's business, engine/runtime.py).
    void stall_tick(Reader& me, int64_t now, int64_t guard, int64_t tick) {
        int64_t oldest = 0;
        bool recovered = false;
        for (auto& kv : streams_) {
            HubStream& s = kv.second;
            if (!s.off_since_ns || now - s.off_since_ns <= tick || s.fd < 0 || s.reader < 0 ||
                readers_[(size_t)s.reader].get() != &me)
                continue;
            if (!has_bytes(s)) continue;
            const int64_t age = now - s.off_since_ns;
            if (age >= guard) {
                std::vector<long long> before = state_of(kv.first, s);
                // (a starved stream keeps its flag and its place in the queue
                // unless this polls it: arm() then queues no second entry)
                arm(kv.first, s);
                if (s.armed & EPOLLIN) {
                    if (s.starved) {
                        s.starved = false;
                        starved_sids_.erase(std::remove(starved_sids_.begin(), starved_sids_.end(), kv.first),
                                            starved_sids_.end());
                    }
                    ++stall_recoveries_;
                    last_stall_.sid = kv.first;
                    last_stall_.age_ns = age;
                    last_stall_.state.swap(before);
                    recovered = true;
                    continue;  // polled again: its bytes wait no more
                }
            }
            oldest = std::max(oldest, age);
        }
        me.oldest_ns.store(oldest, std::memory_order_relaxed);
        if (recovered && !tls_pending_.empty()) wake();
    }

    // (mu_ held)
    void give_back(int i) {
        held_bytes_ -= std::min(held_bytes_, buf_len_[(size_t)i]);
        buf_len_[(size_t)i] = 0;
        free_[cls_[(size_t)i]].push_back(i);
        auto it = streams_.find(owner_[(size_t)i]);
        if (it != streams_.end()) {
            --it->second.held;
            arm(it->first, it->second);
            // decrypted bytes waiting inside OpenSSL never make the socket
            // readable again: have the thread look
            if (tls_pending_.count(it->first)) wake();
        }
        // The pool or the byte budget had run out: poll streams that disarmed,
        // oldest first, as many as one freed buffer can serve (and one spare,
        // in case the first finds its socket drained). Re-arming every starved
        // stream on each release cost the loop O(starved) epoll_ctl calls per
        // buffer and had the losers disarm again at once.
        // Only a re-armed stream with bytes waiting counts: one whose socket
        // was drained when it was disarmed (arm() marks a stream starved over
        // the byte budget whether or not more is coming) gets no event, so
        // it would never read and hand a buffer back to wake the next — with
        // every buffer back, the rest stayed disarmed with their bytes unread
        // (a stall seen with 64 namespace watches and an 8 MiB read-ahead).
        int woken = 0;
        for (size_t left = starved_sids_.size(); left > 0 && woken < HUB_STARVED_WAKE; --left) {
            const int sid2 = starved_sids_.front();
            starved_sids_.pop_front();
            auto jt = streams_.find(sid2);
            if (jt == streams_.end()) continue;
            jt->second.starved = false;
            arm(sid2, jt->second);  // starved again (to the back) if the pool is still short
            if ((jt->second.armed & EPOLLIN) && has_bytes(jt->second)) ++woken;
        }
        if (woken && !tls_pending_.empty()) wake();
    }

  public:
    // release() of many buffers under one lock (the native dispatch)
    void release_many(const int* ids, size_t n) {
        std::lock_guard<std::mutex> g(mu_);
        for (size_t i = 0; i < n; ++i) give_back(ids[i]);
    }

    // From now on the hub frames stream sid's chunked body. `st` is the
    // pipeline's framing state after every byte of sid the loop has taken;
    // the bytes still queued (and one in flight) are framed here first, in
    // order, so the hub's state continues exactly where the pipeline's ends.
    // False: unknown stream, or not framing (already on).
    bool start_framing(int sid, const HubFramer& st) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = streams_.find(sid);
        if (it == streams_.end() || it->second.framer.on) return false;
        HubStream& s = it->second;
        s.framer = st;
        s.framer.on = true;
        for (const HubEntry& e : ready_) {
            if (e.sid != sid || e.buf < 0) continue;
            HubFrame& f = frames_[(size_t)e.buf];
            f.on = true;
            f.upto = 0;
            f.items.clear();
            f.error.clear();
            s.framer.frame(bufs_[(size_t)e.buf].get(), 0, e.len, f);
        }
        if (s.reading && s.reading_buf >= 0) {  // a new buffer being filled (an appended one is queued: done above)
            HubFrame& f = frames_[(size_t)s.reading_buf];
            if (!f.on) {
                f.on = true;
                f.upto = 0;
                f.items.clear();
                f.error.clear();
            }
        }
        return true;
    }

    bool framed(int sid) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = streams_.find(sid);
        return it != streams_.end() && it->second.framer.on;
    }

    // buffer b's framing (the loop, after take() handed b out), or NULL
    const HubFrame* frame_of(int b) const {
        const HubFrame& f = frames_[(size_t)b];
        return f.on ? &f : nullptr;
    }

    // Put taken entries back at the front of the queue, in their order (the
    // native dispatch: reads of a stream after one that needs Python wait
    // for the next take), and have Python take again.
    void requeue(const std::vector<HubEntry>& es) {
        if (es.empty()) return;
        std::lock_guard<std::mutex> g(mu_);
        ready_.insert(ready_.begin(), es.begin(), es.end());
        // taken entries were closed to appends; the queued ones keep theirs
        for (auto& kv : streams_) {
            if (kv.second.open >= 0) kv.second.open += (int)es.size();
        }
        uint64_t one = 1;
        ssize_t r = ::write(py_fd_, &one, 8);
        (void)r;
        ++signals_;
    }

  private:

    void push(const HubEntry& e) {
        const bool was_empty = ready_.empty();
        ready_.push_back(e);
        if (was_empty) {
            uint64_t one = 1;
            ssize_t r = ::write(py_fd_, &one, 8);
            (void)r;
            ++signals_;
        }
    }

    // (mu_ held) a streaming socket (or TLS session) has bytes: read them if
    // a buffer is there for it
    void service(int sid, HubStream& s) {
        if (s.fd < 0 || s.paused) return;
        if (s.phase) {
            drive_setup(sid, s);
            return;
        }
        if (s.want_out) {  // the TLS layer wanted to write: retry the read that asked
            s.want_out = false;
            arm(sid, s);
        }
        if (held_bytes_ >= max_bytes_) {
            ++over_budget_;
            arm(sid, s);  // give_back re-arms
            return;
        }
        if (s.open < 0 && (s.held >= max_held_ || !can_acquire(s.cls, s.held == 0))) {
            if (s.held < max_held_) ++starved_; else ++held_waits_;
            arm(sid, s);  // give_back re-arms
            return;
        }
        read_one(sid, s);
    }

    void loop(Reader& me) {
        epoll_event evs[64];
        std::vector<int> again;
        while (!quit_.load()) {
            const int64_t i0 = mono_ns();
            // the stall guard: asleep no longer than until the next tick, so a
            // stream stranded by a call from the loop thread is seen too
            const int64_t guard = stall_ns_.load(std::memory_order_relaxed);
            const int64_t tick = std::min(HUB_STALL_TICK_NS, guard / 4);
            int wait_ms = -1;
            if (guard) {
                if (!me.next_tick_ns) me.next_tick_ns = i0 + tick;
                wait_ms = me.next_tick_ns > i0 ? (int)((me.next_tick_ns - i0 + 999999) / 1000000) : 0;
            }
            int n = epoll_wait(me.ep, evs, 64, wait_ms);
            const int64_t i1 = mono_ns();
            idle_ns_.fetch_add(i1 - i0, std::memory_order_relaxed);
            if (n < 0) {
                if (errno == EINTR) continue;
                return;
            }
            std::unique_lock<std::mutex> lk(mu_);
            cur_lock_ = &lk;  // read_one drops it around recv
            if (!guard) {
                me.next_tick_ns = 0;
                if (me.oldest_ns.load(std::memory_order_relaxed)) me.oldest_ns.store(0, std::memory_order_relaxed);
            } else if (i1 >= me.next_tick_ns) {
                me.next_tick_ns = i1 + tick;
                stall_tick(me, i1, guard, tick);
            }
            for (int i = 0; i < n; ++i) {
                const uint32_t sid = evs[i].data.u32;
                if (sid == UINT32_MAX) {
                    uint64_t v;
                    ssize_t r = ::read(me.wake_fd, &v, 8);
                    (void)r;
                    continue;
                }
                auto it = streams_.find((int)sid);
                if (it != streams_.end()) service((int)sid, it->second);
            }
            // TLS sessions holding decrypted bytes the socket no longer signals
            // (this thread's streams: a stream is read by its own thread only)
            again.assign(tls_pending_.begin(), tls_pending_.end());
            for (int sid : again) {
                auto it = streams_.find(sid);
                if (it == streams_.end()) {
                    tls_pending_.erase(sid);
                    continue;
                }
                HubStream& s = it->second;
                if (s.reader < 0 || readers_[(size_t)s.reader].get() != &me) continue;
                if (!s.paused && held_bytes_ < max_bytes_ &&
                    (s.open >= 0 || (can_acquire(s.cls, s.held == 0) && s.held < max_held_)))
                    read_one(sid, s);
            }
        }
    }

    // (mu_ held via cur_lock_) whatever the socket holds now, up to one
    // buffer. While the loop has not taken the stream's newest buffer, reads
    // append to it: a busy loop then gets few large buffers (one sink call
    // each) instead of one per socket read. The recv itself runs without the
    // lock — the loop's take() and release() do not wait for a multi-megabyte
    // copy (profiles/cprofile_loop_gpu_box.md): the socket stays open
    // (remove() defers to us), the bytes past the entry's length are ours
    // alone, and take() leaves an entry we are appending to queued.
    void read_one(int sid, HubStream& s) {
        const bool append = s.open >= 0;
        int b;
        size_t len;
        if (append) {
            b = ready_[(size_t)s.open].buf;
            len = ready_[(size_t)s.open].len;
        } else {
            if (s.held >= max_held_) {  // wait for the loop to hand one back
                ++held_waits_;
                arm(sid, s);
                return;
            }
            s.cls = std::max(s.cls, fair_cls());  // more streams than when it grew: back to its share
            b = acquire(s.cls, s.held == 0);
            if (b < 0) {  // the pool is short: give_back re-arms
                ++starved_;
                arm(sid, s);
                return;
            }
            len = 0;
            owner_[(size_t)b] = sid;
            ++s.held;
        }
        char* p = bufs_[(size_t)b].get();
        const size_t cap = cap_[(size_t)b];
        HubFrame& fr = frames_[(size_t)b];
        if (!append) {  // a new buffer: framed iff its stream is, from its first byte
            fr.on = s.framer.on;
            fr.upto = 0;
            fr.items.clear();
            fr.error.clear();
        }
        // framed here, outside the lock, only if it already was: a
        // start_framing() meanwhile (which frames what is queued, under the
        // lock) leaves this read's bytes to the framing after the re-lock
        const bool frame_unlocked = fr.on;
        s.reading_buf = b;
        if (s.rx) size_ring(s, cap);
        const size_t budget = held_bytes_ < max_bytes_ ? max_bytes_ - held_bytes_ : 0;
        int64_t t = 0;
        int err = -1;  // -1: still open
        std::string why;
        size_t got = 0;
        bool over = false, want_write = false;
        s.reading = true;
        cur_lock_->unlock();
        const int64_t t_recv = mono_ns();
        int64_t in_frame = 0, rc_ns = 0, dec_ns = 0;
        if (s.rx) rx_read(s, p, len, cap, budget, got, t, err, why, over, rc_ns, dec_ns);
        while (!s.rx && len < cap) {
            const ssize_t k = stream_read(s, p + len, cap - len, why, want_write);
            if (k > 0) {
                if (!t) t = mono_ns();
                len += (size_t)k;
                got += (size_t)k;
                reads_.fetch_add(1, std::memory_order_relaxed);
                if (got >= budget) {  // budget spent: the rest waits in the socket
                    over = true;
                    break;
                }
                continue;
            }
            if (k == 0) err = 0;
            if (k == -2) err = 1;
            break;
        }
        const bool tls_more =
            err < 0 && (s.rx ? s.rx->whole_record() || (s.rx->eof && s.rx->pending()) : s.ssl && SSL_pending(s.ssl) > 0);
        const int64_t t_frame = mono_ns();
        recv_ns_.fetch_add(s.rx ? rc_ns : t_frame - t_recv - in_frame, std::memory_order_relaxed);
        if (dec_ns) decrypt_ns_.fetch_add(dec_ns, std::memory_order_relaxed);
        recv_bytes_.fetch_add((long long)got, std::memory_order_relaxed);
        if (frame_unlocked && len > fr.upto) {
            s.framer.frame(p, fr.upto, len, fr);
            in_frame += mono_ns() - t_frame;
        }
        if (in_frame) {
            framed_reads_.fetch_add(1, std::memory_order_relaxed);
            frame_ns_.fetch_add(in_frame, std::memory_order_relaxed);
        }
        cur_lock_->lock();
        s.reading = false;
        s.reading_buf = -1;
        if (s.rx) count_ring(s);  // (a split handshake message's buffer may have grown)
        if (fr.on && len > fr.upto) {  // framing began during the recv
            s.framer.frame(p, fr.upto, len, fr);
            framed_reads_.fetch_add(1, std::memory_order_relaxed);
        }
        if (want_write) s.want_out = true;
        if (got) s.last_ns = mono_ns();
        held_bytes_ += got;
        buf_len_[(size_t)b] = len;
        if (over) ++over_budget_;
        if (s.removed) {  // remove() came while we were in recv: drop the stream now
            if (append) {
                ready_.erase(ready_.begin() + s.open);
            }
            give_back(b);
            if (s.fd >= 0) epoll_ctl(ep_of(s), EPOLL_CTL_DEL, s.fd, nullptr);
            release_stream(s);
            drop_from_reader(s);
            tls_pending_.erase(sid);
            errors_.erase(sid);
            streams_.erase(sid);  // s is gone from here on
            reopen();
            signal_if_deferred();
            return;
        }
        if (s.ssl) {
            if (tls_more) tls_pending_.insert(sid); else tls_pending_.erase(sid);
        }
        if (len >= cap && s.cls > fair_cls()) {
            --s.cls;  // filled before the loop took it: read more at a time (up to its share)
        } else if (!append && got < class_bytes(s.cls) / 16 && s.cls < HUB_CLASSES - 1) {
            ++s.cls;  // mostly empty: a smaller buffer will do
        }
        if (append) {
            HubEntry& e = ready_[(size_t)s.open];  // take() and remove() keep our entry's index current
            e.len = len;  // keeps the first read's time: latency counts from the oldest byte
            if (len >= cap) s.open = -1;
        } else if (len) {
            push(HubEntry{sid, b, len, t, 0});
            s.open = len < cap ? (int)ready_.size() - 1 : -1;
        } else {
            free_[cls_[(size_t)b]].push_back(b);
            buf_len_[(size_t)b] = 0;
            --s.held;
        }
        signal_if_deferred();
        arm(sid, s);
        if (err >= 0)  // the peer closed or the socket failed: no more polling
            finish(sid, s, err == 0 ? 0 : -1, why);
        // (streams the pool can no longer serve are disarmed by service() on
        // their next event, not all at once here: O(1) per read with many streams)
    }

    // (mu_ held) take() left an entry we were appending to queued: wake Python for it
    void signal_if_deferred() {
        if (!deferred_ || ready_.empty()) {
            deferred_ = false;
            return;
        }
        deferred_ = false;
        uint64_t one = 1;
        ssize_t r = ::write(py_fd_, &one, 8);
        (void)r;
        ++signals_;
    }

    size_t buf_bytes_;
    const size_t pool_bytes_;  // memory of all allocated buffers, at most (nbufs * buf_bytes)
    size_t alloc_bytes_ = 0;
    std::vector<std::unique_ptr<char[]>> bufs_;
    std::vector<HubFrame> frames_;  // per buffer id: its framing, when its stream is hub-framed
    std::vector<size_t> cap_;    // each buffer id's allocated size (0: none)
    std::vector<int> cls_;       // ... and its class
    std::vector<int> free_[HUB_CLASSES];  // allocated, not in use, per class
    std::vector<int> spare_;     // ids without memory
    std::vector<int> owner_;  // stream id of each buffer in use
    std::vector<size_t> buf_len_;  // bytes read into each buffer in use (counted in held_bytes_)
    const size_t max_bytes_;  // read-ahead budget over all streams
    size_t held_bytes_ = 0;
    size_t ring_bytes_ = 0;   // TLS ciphertext rings (Tls13Rx), within pool_bytes_ with the buffers
    size_t rx_streams_ = 0;   // streams whose records the hub opens (fair_cls)
    bool deferred_ = false;  // take() left an entry being appended to queued (signal when done)
    // the running reader thread's hold on mu_ (loop(); read_one drops it around recv)
    static inline thread_local std::unique_lock<std::mutex>* cur_lock_ = nullptr;
    static inline thread_local std::vector<RecSpan> recs_;  // a reader thread's scratch (TLS records)
    std::vector<HubEntry> ready_;
    std::deque<int> starved_sids_;  // streams arm() left off for want of a buffer or byte budget (FIFO)
    std::unordered_map<int, HubStream> streams_;
    std::unordered_map<int, std::string> errors_;
    std::unordered_set<int> tls_pending_;
    int next_sid_ = 1;
    // Reader threads: each polls its own streams (a stream stays with the
    // thread it was given, so its reads stay in order); they share the pool,
    // the ready queue and the one eventfd the loop waits on — the loop takes
    // every thread's reads in one dispatch. More than one pays with many
    // watch streams, where one thread's recv (+ framing) was the bound.
    std::vector<std::unique_ptr<Reader>> readers_;
    int py_fd_ = -1;
    std::mutex mu_;
    std::atomic<bool> quit_{false};
    std::atomic<long long> reads_{0}, signals_{0}, starved_{0}, over_budget_{0};
    std::atomic<long long> framed_reads_{0};  // reads whose bytes the hub framed (start_framing)
    // where the reader thread's time goes: in recv() (the kernel's copy into
    // our buffer, and EAGAIN probes) and in framing outside the lock
    std::atomic<long long> recv_ns_{0}, frame_ns_{0}, recv_bytes_{0};
    std::atomic<long long> idle_ns_{0};     // the reader threads in epoll_wait (nothing to read, or no buffer)
    std::atomic<long long> held_waits_{0};  // a stream with bytes waited: it held max_held buffers the loop had not released
    long long ring_resizes_ = 0;            // (mu_) TLS rings grown or shrunk
    // TLS record layer (tls13.inc): streams taken over / left on SSL_read,
    // ciphertext bytes received, time opening records (reader thread, waits
    // for the pool included); the pool's own threads report in tls_pool()
    bool tls_records_ = true;
    std::unique_ptr<CryptoPool> pool_;
    std::atomic<long long> tls_taken_{0}, tls_kept_{0}, tls_ct_bytes_{0}, decrypt_ns_{0};
    std::array<long long, 4> tls_done_{};  // (mu_) tls_records() of streams already released
    int max_held_ = HUB_MAX_HELD;  // (mu_) read-ahead per stream in buffers
    // the stall guard (set_stall_guard): its setting, streams it re-armed, the last of them
    std::atomic<int64_t> stall_ns_{0};
    std::atomic<long long> stall_recoveries_{0};
    HubStall last_stall_;  // (mu_)
};

// A stream bound to a fused Pipeline (engine.inc): take_dispatch() runs its
// buffers through the pipeline here, with no Python call per read.
struct HubBinding {
    PyObject* pipeline;  // PipelineObject, owned reference
    bool framed;         // HTTP-chunk framed body (feed_chunked) or not (feed)
    bool hub_framing = false;  // the hub frames this chunked body (start_framing)
};

struct ReaderHubObject {
    PyObject_HEAD
    ReaderHub* hub;
    std::unordered_map<int, HubBinding>* bound;
    bool frame;  // hand bound chunked bodies' framing to the hub thread (start_framing)
    long long merged;   // reads merged into an earlier read's batch of the same stream (take_dispatch)
    long long batches;  // pipeline calls take_dispatch made for bound streams
};

PyObject* ReaderHub_new(PyTypeObject* type, PyObject*, PyObject*) {
    ReaderHubObject* self = (ReaderHubObject*)type->tp_alloc(type, 0);
    if (self) {
        self->hub = nullptr;
        self->bound = new std::unordered_map<int, HubBinding>();
        self->frame = true;
        self->merged = self->batches = 0;
    }
    return (PyObject*)self;
}

void hub_unbind_all(ReaderHubObject* self) {
    if (!self->bound) return;
    std::unordered_map<int, HubBinding> old;
    old.swap(*self->bound);
    for (auto& kv : old) Py_DECREF(kv.second.pipeline);
}

int ReaderHub_init(ReaderHubObject* self, PyObject* args, PyObject* kwds) {
    static const char* kwlist[] = {"buf_bytes", "nbufs", "max_bytes", "frame", nullptr};
    Py_ssize_t buf_bytes, max_bytes = 0;
    int nbufs, frame = 1;
    if (!PyArg_ParseTupleAndKeywords(args, kwds, "ni|np", const_cast<char**>(kwlist), &buf_bytes, &nbufs, &max_bytes,
                                     &frame))
        return -1;
    self->frame = frame != 0;
    if (buf_bytes < 4096 || buf_bytes > (1 << 28) || nbufs < 2 || nbufs > 1024 || max_bytes < 0) {
        PyErr_SetString(PyExc_ValueError,
                        "ReaderHub(buf_bytes in [4 KiB, 256 MiB], nbufs in [2, 1024], max_bytes >= 0)");
        return -1;
    }
    delete self->hub;
    self->hub = new ReaderHub((size_t)buf_bytes, nbufs, (size_t)max_bytes);
    if (!self->hub->ok()) {
        delete self->hub;
        self->hub = nullptr;
        PyErr_SetFromErrno(PyExc_OSError);
        return -1;
    }
    return 0;
}

void ReaderHub_dealloc(ReaderHubObject* self) {
    hub_unbind_all(self);
    delete self->bound;
    if (self->hub) {
        Py_BEGIN_ALLOW_THREADS
        delete self->hub;  // joins the reader thread (it never takes the GIL)
        Py_END_ALLOW_THREADS
    }
    Py_TYPE(self)->tp_free((PyObject*)self);
}

#define HUB_OR_FAIL(self)                                                  \
    if (!(self)->hub) {                                                    \
        PyErr_SetString(PyExc_RuntimeError, "ReaderHub is closed");        \
        return nullptr;                                                    \
    }

PyObject* ReaderHub_fileno(ReaderHubObject* self, PyObject*) {
    HUB_OR_FAIL(self);
    return PyLong_FromLong(self->hub->py_fd());
}

PyObject* ReaderHub_add(ReaderHubObject* self, PyObject* arg) {
    HUB_OR_FAIL(self);
    int fd = (int)PyLong_AsLong(arg);
    if (fd < 0) {
        if (!PyErr_Occurred()) PyErr_SetString(PyExc_ValueError, "fd");
        return nullptr;
    }
    int fl = fcntl(fd, F_GETFL);
    if (fl < 0 || fcntl(fd, F_SETFL, fl | O_NONBLOCK) < 0) return PyErr_SetFromErrno(PyExc_OSError);
    return PyLong_FromLong(self->hub->add(fd));
}

PyTypeObject TlsCtxType = {PyVarObject_HEAD_INIT(nullptr, 0)};

// add_tls(fd, context, host, request) -> sid: the hub owns fd from here on
PyObject* ReaderHub_add_tls(ReaderHubObject* self, PyObject* args) {
    HUB_OR_FAIL(self);
    int fd;
    PyObject* ctx;
    const char* host;
    const char* req;
    Py_ssize_t reqn;
    if (!PyArg_ParseTuple(args, "iO!sy#", &fd, &TlsCtxType, &ctx, &host, &req, &reqn)) return nullptr;
    int fl = fcntl(fd, F_GETFL);
    if (fl < 0 || fcntl(fd, F_SETFL, fl | O_NONBLOCK) < 0) return PyErr_SetFromErrno(PyExc_OSError);
    TlsCtxObject* c = (TlsCtxObject*)ctx;
    std::string error;
    const int sid = self->hub->add_tls(fd, c->ctx, c->verify, host, std::string(req, (size_t)reqn), error);
    if (sid < 0) {
        ::close(fd);
        PyErr_SetString(PyExc_OSError, error.c_str());
        return nullptr;
    }
    return PyLong_FromLong(sid);
}

PyObject* ReaderHub_error_text(ReaderHubObject* self, PyObject* arg) {
    HUB_OR_FAIL(self);
    int sid = (int)PyLong_AsLong(arg);
    if (PyErr_Occurred()) return nullptr;
    const std::string e = self->hub->error_text(sid);
    return PyUnicode_DecodeUTF8(e.data(), (Py_ssize_t)e.size(), "replace");
}

void hub_unbind(ReaderHubObject* self, int sid) {
    auto it = self->bound->find(sid);
    if (it == self->bound->end()) return;
    PyObject* pl = it->second.pipeline;
    self->bound->erase(it);
    Py_DECREF(pl);
}

PyObject* ReaderHub_remove(ReaderHubObject* self, PyObject* arg) {
    HUB_OR_FAIL(self);
    int sid = (int)PyLong_AsLong(arg);
    if (PyErr_Occurred()) return nullptr;
    hub_unbind(self, sid);
    self->hub->remove(sid);
    Py_RETURN_NONE;
}

// bind(sid, pipeline, framed): from now on take_dispatch() feeds this
// stream's buffers to the fused Pipeline itself (feed_chunked / feed)
PyObject* ReaderHub_bind(ReaderHubObject* self, PyObject* args) {
    HUB_OR_FAIL(self);
    int sid, framed;
    PyObject* pl;
    if (!PyArg_ParseTuple(args, "iO!p", &sid, &PipelineType, &pl, &framed)) return nullptr;
    hub_unbind(self, sid);
    Py_INCREF(pl);
    (*self->bound)[sid] = HubBinding{pl, framed != 0, false};
    Py_RETURN_NONE;
}

PyObject* ReaderHub_unbind(ReaderHubObject* self, PyObject* arg) {
    int sid = (int)PyLong_AsLong(arg);
    if (PyErr_Occurred()) return nullptr;
    hub_unbind(self, sid);
    // a hub-framed body cannot go back to raw reads: its pipeline's own
    // framing state stopped where the hub's began
    if (self->hub && self->hub->framed(sid)) self->hub->remove(sid);
    Py_RETURN_NONE;
}

PyObject* ReaderHub_pause(ReaderHubObject* self, PyObject* args) {
    HUB_OR_FAIL(self);
    int sid, paused;
    if (!PyArg_ParseTuple(args, "ip", &sid, &paused)) return nullptr;
    self->hub->pause(sid, paused);
    Py_RETURN_NONE;
}

// take() -> [(sid, buf, memoryview | None, read_ns, err)] in arrival order;
// every buf >= 0 must be handed back with release(buf) once consumed, and the
// view must not be used after that.
PyObject* ReaderHub_take(ReaderHubObject* self, PyObject*) {
    HUB_OR_FAIL(self);
    std::vector<HubEntry> got = self->hub->take();
    PyObject* out = PyList_New((Py_ssize_t)got.size());
    if (!out) return nullptr;
    for (size_t i = 0; i < got.size(); ++i) {
        const HubEntry& e = got[i];
        PyObject* view;
        if (e.buf >= 0) {
            view = PyMemoryView_FromMemory(const_cast<char*>(self->hub->buf(e.buf)), (Py_ssize_t)e.len, PyBUF_READ);
        } else {
            Py_INCREF(Py_None);
            view = Py_None;
        }
        PyObject* t = view ? Py_BuildValue("(iiNLi)", e.sid, e.buf, view, (long long)e.read_ns, e.err) : nullptr;
        if (!t) {
            Py_DECREF(out);
            return nullptr;
        }
        PyList_SET_ITEM(out, (Py_ssize_t)i, t);
    }
    return out;
}

// take_dispatch() -> (items, touched): take() with the buffers of bound
// streams run through their Pipeline right here and handed back to the pool.
// Only what needs Python comes back in `items`, in arrival order:
//   (sid, buf, view | None, read_ns, err)   as take(): unbound streams and
//                                           end-of-stream entries
//   (sid, -2, result, read_ns, body_done)   a bound read whose result has
//                                           control events, log lines or
//                                           submissions, or that ended the
//                                           body; result is feed()'s tuple or
//                                           the exception it raised
// A bound stream's entries after such a read go back to the queue (requeue)
// and are fed natively on the next take, once Python has seen that read.
// `touched`: every sid that had data (its last-activity time).
// Reads of bound streams are batched (pl_run_group, engine.inc): consecutive
// ones, each Pipeline at most once, up to this many bytes, go through the
// decode pool as one batch of lines.
constexpr size_t HUB_GROUP_BYTES = 4u << 20;

// Whether a read's bytes end the watch body: its hub framing holds the
// terminating chunk (or a framing error), or — bytes the pipeline frames
// itself — they end in the terminating chunk "0\r\n\r\n" (a JSON line's
// chunk ends "\n\r\n", so a match is the terminator; a false match would
// only cost a separate call).
bool read_ends_body(const char* data, size_t len, const HubFrame* fr) {
    if (fr) {
        for (auto it = fr->items.rbegin(); it != fr->items.rend(); ++it)
            if (it->kind == HI_DONE || it->kind == HI_ERROR) return true;
        return false;
    }
    return len >= 5 && std::memcmp(data + len - 5, "0\r\n\r\n", 5) == 0;
}

PyObject* ReaderHub_take_dispatch(ReaderHubObject* self, PyObject*) {
    HUB_OR_FAIL(self);
    std::vector<HubEntry> got = self->hub->take();
    PyObject* items = PyList_New(0);
    PyObject* touched = PyList_New(0);
    if (!items || !touched) {
        Py_XDECREF(items);
        Py_XDECREF(touched);
        self->hub->requeue(got);  // nothing consumed: all of it on the next take
        return nullptr;
    }
    std::vector<int> held;        // sids with an attention item: their later entries wait for the next take
    std::vector<HubEntry> again;  // ... those entries, in order
    std::unordered_set<int> seen;  // sids already in touched
    auto contains = [](const std::vector<int>& v, int sid) {
        for (int x : v)
            if (x == sid) return true;
        return false;
    };
    bool failed = false;
    std::vector<GroupRead> group;
    std::vector<int> gsid, gbuf;
    std::vector<PyObject*> results;
    size_t gbytes = 0;
    // run the pending group; its reads that need Python become items (in order)
    auto flush = [&]() {
        if (group.empty()) return;
        self->batches += (long long)group.size();
        pl_run_group(group, results);
        self->hub->release_many(gbuf.data(), gbuf.size());
        for (size_t k = 0; k < group.size(); ++k) {
            GroupRead& r = group[k];
            PyObject* res = results[k];
            const bool done = r.framed && r.pl->chunk.done();
            Py_DECREF(r.pl);
            if (!res || failed) {  // out of memory
                failed = true;
                Py_XDECREF(res);
                continue;
            }
            bool attention = done || !r.ok;  // !ok: res is the exception the read raised
            if (!attention) {
                PyObject* ctrl = PyTuple_GET_ITEM(res, 0);
                attention = PyList_GET_SIZE(ctrl) > 0 || PyTuple_GET_ITEM(res, 2) != Py_None ||
                            PyTuple_GET_ITEM(res, 3) != Py_None;
            }
            if (!attention) {
                Py_DECREF(res);
                continue;
            }
            held.push_back(gsid[k]);
            PyObject* t = Py_BuildValue("(iiNLi)", gsid[k], -2, res, r.read_ns, done ? 1 : 0);
            if (!t || PyList_Append(items, t) < 0) failed = true;
            Py_XDECREF(t);
        }
        group.clear();
        gsid.clear();
        gbuf.clear();
        gbytes = 0;
    };
    for (size_t i = 0; i < got.size(); ++i) {
        const HubEntry& e = got[i];
        if (failed) {  // out of memory building the lists: the rest waits for the next take
            again.push_back(e);
            continue;
        }
        if (e.buf >= 0 && seen.insert(e.sid).second) {
            PyObject* s = PyLong_FromLong(e.sid);
            if (!s || PyList_Append(touched, s) < 0) failed = true;
            Py_XDECREF(s);
        }
        const bool is_bound = self->bound->count(e.sid) > 0;
        if (is_bound && e.buf >= 0 && !contains(held, e.sid) && contains(gsid, e.sid)) {
            // a later read of a stream already in this batch: merged into its
            // call (GroupRead::more, engine.inc) when its submits are native
            size_t k = 0;
            while (gsid[k] != e.sid) ++k;
            GroupRead& r = group[k];
            const HubFrame* fr = self->hub->frame_of(e.buf);
            // never past the end of the body: the read that ends it needs
            // Python (the reflector reconnects) before anything after it
            const bool prev_ends = r.more.empty() ? read_ends_body(r.data, r.len, r.frame)
                                                  : read_ends_body(r.more.back().data, r.more.back().len,
                                                                   r.more.back().frame);
            if (r.pl->notifier && !prev_ends && !!fr == !!r.frame && (!fr || fr->upto == e.len)) {
                r.more.push_back(GroupRead::Part{self->hub->buf(e.buf), e.len, (long long)e.read_ns, fr});
                ++self->merged;
                gbuf.push_back(e.buf);
                gbytes += e.len;
                if (gbytes >= HUB_GROUP_BYTES) flush();
                continue;
            }
            flush();  // its previous read first: it may need Python before this one
        }
        if (is_bound && contains(held, e.sid)) {
            // after a read that needs Python: back in the queue, fed natively
            // on the next take, after Python has seen that read (a bound
            // body never goes to Python raw: the hub may be framing it)
            again.push_back(e);
            continue;
        }
        auto it = e.buf >= 0 && is_bound ? self->bound->find(e.sid) : self->bound->end();
        if (it == self->bound->end()) {
            flush();  // earlier reads' items come first
            if (failed) {
                again.push_back(e);
                continue;
            }
            PyObject* view = e.buf >= 0 ? PyMemoryView_FromMemory(const_cast<char*>(self->hub->buf(e.buf)),
                                                                  (Py_ssize_t)e.len, PyBUF_READ)
                                        : (Py_INCREF(Py_None), Py_None);
            PyObject* t = view ? Py_BuildValue("(iiNLi)", e.sid, e.buf, view, (long long)e.read_ns, e.err) : nullptr;
            if (!t || PyList_Append(items, t) < 0) {
                failed = true;
                again.push_back(e);
            }
            Py_XDECREF(t);
            continue;
        }
        GroupRead r;
        r.pl = (PipelineObject*)it->second.pipeline;
        Py_INCREF(r.pl);  // the batch may call Python (and drop the GIL): an unbind meanwhile must not free it
        r.data = self->hub->buf(e.buf);
        r.len = e.len;
        r.read_ns = (long long)e.read_ns;
        r.framed = it->second.framed;
        r.frame = self->hub->frame_of(e.buf);
        if (r.frame && r.frame->upto != e.len) {  // cannot happen (read_one frames before it queues)
            Py_DECREF(r.pl);
            PyErr_Format(PyExc_RuntimeError, "reader hub: buffer framed to %zu of %zu bytes", r.frame->upto, e.len);
            failed = true;
            again.push_back(e);
            continue;
        }
        group.push_back(r);
        gsid.push_back(e.sid);
        gbuf.push_back(e.buf);
        gbytes += e.len;
        if (gbytes >= HUB_GROUP_BYTES) flush();
    }
    flush();
    self->hub->requeue(again);
    // chunked bodies the hub does not frame yet: hand it each pipeline's
    // framing state now that every taken byte of the stream went through it
    for (int sid : seen) {
        if (!self->frame) break;
        auto it = self->bound->find(sid);
        if (it == self->bound->end() || !it->second.framed || it->second.hub_framing) continue;
        PipelineObject* pl = (PipelineObject*)it->second.pipeline;
        if (pl->chunk.done()) continue;
        HubFramer st;
        st.chunk = pl->chunk;
        st.in_line = !pl->partial->empty();
        it->second.hub_framing = self->hub->start_framing(sid, st);
    }
    if (failed) {
        // anything already in items holds buffers: hand them back before failing
        for (Py_ssize_t i = 0; i < PyList_GET_SIZE(items); ++i) {
            PyObject* t = PyList_GET_ITEM(items, i);
            const long b = PyLong_AsLong(PyTuple_GET_ITEM(t, 1));
            if (b >= 0) {
                PyObject* v = PyTuple_GET_ITEM(t, 2);
                if (PyMemoryView_Check(v)) {
                    PyObject* r = PyObject_CallMethod(v, "release", nullptr);
                    Py_XDECREF(r);
                }
                self->hub->release((int)b);
            }
        }
        Py_DECREF(items);
        Py_DECREF(touched);
        if (!PyErr_Occurred()) PyErr_NoMemory();
        return nullptr;
    }
    return Py_BuildValue("(NN)", items, touched);
}

PyObject* ReaderHub_release(ReaderHubObject* self, PyObject* arg) {
    HUB_OR_FAIL(self);
    int b = (int)PyLong_AsLong(arg);
    if (PyErr_Occurred()) return nullptr;
    if (b >= 0) self->hub->release(b);
    Py_RETURN_NONE;
}

PyObject* ReaderHub_stats(ReaderHubObject* self, PyObject*) {
    HUB_OR_FAIL(self);
    ReaderHub& h = *self->hub;
    const auto mem = h.memory();
    PyObject* d = Py_BuildValue("{s:L,s:L,s:L,s:L,s:n,s:n,s:n,s:L,s:L,s:L,s:L,s:L,s:L,s:L,s:L,s:L,s:L,s:L,s:L}", "reads", h.reads(),
                                "signals", h.wakeups(), "starved", h.starved(), "over_budget", h.over_budget(),
                                "max_bytes", (Py_ssize_t)h.max_bytes(), "allocated_bytes", (Py_ssize_t)mem[0],
                                "held_bytes", (Py_ssize_t)mem[1], "framed_reads", h.framed_reads(),
                                "merged_reads", self->merged, "dispatch_batches", self->batches, "depth",
                                (long long)h.depth(), "recv_ns", h.recv_ns(), "frame_ns", h.frame_ns(), "recv_bytes",
                                h.recv_bytes(), "idle_ns", h.idle_ns(), "held_waits", h.held_waits(), "oldest_unread_ns",
                                (long long)h.oldest_unread_ns(), "stall_recoveries", h.stall_recoveries(), "stall_guard_ns",
                                (long long)h.stall_guard_ns());
    if (!d) return nullptr;
    const auto rec = h.tls_records();
    const auto pool = h.tls_pool();
    PyObject* pl = PyList_New((Py_ssize_t)pool.size());
    for (size_t i = 0; pl && i < pool.size(); ++i)
        PyList_SET_ITEM(pl, (Py_ssize_t)i, Py_BuildValue("(LL)", pool[i].first, pool[i].second));
    PyObject* extra = pl ? Py_BuildValue("{s:n,s:L,s:L,s:L,s:L,s:L,s:L,s:L,s:L,s:L,s:L,s:N}", "tls_ring_bytes",
                                         (Py_ssize_t)mem[2], "tls_ring_resizes", h.ring_resizes(), "tls_taken", h.tls_taken(),
                                         "tls_kept", h.tls_kept(), "tls_ct_bytes", h.tls_ct_bytes(), "decrypt_ns",
                                         h.decrypt_ns(), "tls_records", rec[0], "tls_pooled_records", rec[1],
                                         "tls_key_updates", rec[2], "tls_tickets", rec[3], "tls_pool_wait_ns",
                                         h.tls_pool_wait_ns(), "tls_pool", pl)
                         : nullptr;
    if (!extra || PyDict_Update(d, extra) < 0) {
        Py_XDECREF(extra);
        Py_DECREF(d);
        return nullptr;
    }
    Py_DECREF(extra);
    return d;
}

// set_tls(records, threads): TLS 1.3 streams' records read and opened by the
// hub itself (tls13.inc) — on `threads` pool threads besides the reader
// thread — or left to SSL_read (records=False). Before streams are added.
PyObject* ReaderHub_set_tls(ReaderHubObject* self, PyObject* args) {
    HUB_OR_FAIL(self);
    int records, threads;
    if (!PyArg_ParseTuple(args, "pi", &records, &threads)) return nullptr;
    if (threads < 0 || threads > 32) {
        PyErr_SetString(PyExc_ValueError, "TLS threads: 0..32");
        return nullptr;
    }
    self->hub->set_tls(records, threads);
    Py_RETURN_NONE;
}

// set_depth(n): read-ahead per stream, in buffers queued or held (2..8)
PyObject* ReaderHub_set_depth(ReaderHubObject* self, PyObject* arg) {
    HUB_OR_FAIL(self);
    const long n = PyLong_AsLong(arg);
    if (n == -1 && PyErr_Occurred()) return nullptr;
    if (n < HUB_MAX_HELD || n > HUB_MAX_DEPTH) {
        PyErr_Format(PyExc_ValueError, "read-ahead depth: %d..%d buffers", HUB_MAX_HELD, HUB_MAX_DEPTH);
        return nullptr;
    }
    self->hub->set_depth((int)n);
    Py_RETURN_NONE;
}

PyObject* ReaderHub_thread_id(ReaderHubObject* self, PyObject*) {
    HUB_OR_FAIL(self);
    return PyLong_FromLong(self->hub->tid());
}

// set_readers(n): n reader threads in all (1..8), each polling its share of
// the streams added from now on (the one with the fewest first) — for many
// watch streams, where one thread's recv and framing were the bound. False if
// it could not (threads never go away while the hub runs).
PyObject* ReaderHub_set_readers(ReaderHubObject* self, PyObject* arg) {
    HUB_OR_FAIL(self);
    const long n = PyLong_AsLong(arg);
    if (n == -1 && PyErr_Occurred()) return nullptr;
    if (n < 1 || n > HUB_MAX_READERS) {
        PyErr_Format(PyExc_ValueError, "reader threads: 1..%d", HUB_MAX_READERS);
        return nullptr;
    }
    return PyBool_FromLong(self->hub->set_readers((int)n));
}

// thread_ids() -> [kernel thread id] of every reader thread (placement)
PyObject* ReaderHub_thread_ids(ReaderHubObject* self, PyObject*) {
    HUB_OR_FAIL(self);
    const int n = self->hub->readers();
    std::vector<int> ids;
    Py_BEGIN_ALLOW_THREADS
    for (int i = 0; i < n; ++i) ids.push_back(self->hub->tid(i));
    Py_END_ALLOW_THREADS
    PyObject* l = PyList_New((Py_ssize_t)ids.size());
    for (size_t i = 0; l && i < ids.size(); ++i) PyList_SET_ITEM(l, (Py_ssize_t)i, PyLong_FromLong(ids[i]));
    return l;
}

// last_read(sid) -> time.monotonic() seconds when the stream's last read with
// bytes ended (0.0: none yet, or unknown): a bound stream's activity without
// a Python call per dispatch (net/reader.py, the reflectors' idle checks)
PyObject* ReaderHub_last_read(ReaderHubObject* self, PyObject* arg) {
    HUB_OR_FAIL(self);
    const long sid = PyLong_AsLong(arg);
    if (sid == -1 && PyErr_Occurred()) return nullptr;
    return PyFloat_FromDouble((double)self->hub->last_read((int)sid) * 1e-9);
}

// stream_state(sid) -> tuple of ints (ReaderHub::stream_state), () if unknown
PyObject* ReaderHub_stream_state(ReaderHubObject* self, PyObject* arg) {
    HUB_OR_FAIL(self);
    const long sid = PyLong_AsLong(arg);
    if (sid == -1 && PyErr_Occurred()) return nullptr;
    const std::vector<long long> v = self->hub->stream_state((int)sid);
    PyObject* t = PyTuple_New((Py_ssize_t)v.size());
    for (size_t i = 0; t && i < v.size(); ++i) PyTuple_SET_ITEM(t, (Py_ssize_t)i, PyLong_FromLongLong(v[i]));
    return t;
}

// set_stall_guard(seconds): ReaderHub::set_stall_guard (0 = off)
PyObject* ReaderHub_set_stall_guard(ReaderHubObject* self, PyObject* arg) {
    HUB_OR_FAIL(self);
    const double s = PyFloat_AsDouble(arg);
    if (s == -1.0 && PyErr_Occurred()) return nullptr;
    if (!(s >= 0) || s > 86400) {
        PyErr_SetString(PyExc_ValueError, "stall guard: 0 (off) .. 86400 seconds");
        return nullptr;
    }
    self->hub->set_stall_guard(s);
    Py_RETURN_NONE;
}

// oldest_unread() -> seconds (ReaderHub::oldest_unread_ns), 0.0 with none
PyObject* ReaderHub_oldest_unread(ReaderHubObject* self, PyObject*) {
    HUB_OR_FAIL(self);
    return PyFloat_FromDouble((double)self->hub->oldest_unread_ns() * 1e-9);
}

PyObject* ReaderHub_stall_recoveries(ReaderHubObject* self, PyObject*) {
    HUB_OR_FAIL(self);
    return PyLong_FromLongLong(self->hub->stall_recoveries());
}

// last_stall() -> (sid, seconds it had been off, its stream_state before the re-arm), None if none
PyObject* ReaderHub_last_stall(ReaderHubObject* self, PyObject*) {
    HUB_OR_FAIL(self);
    const HubStall st = self->hub->last_stall();
    if (!st.sid) Py_RETURN_NONE;
    PyObject* t = PyTuple_New((Py_ssize_t)st.state.size());
    for (size_t i = 0; t && i < st.state.size(); ++i) PyTuple_SET_ITEM(t, (Py_ssize_t)i, PyLong_FromLongLong(st.state[i]));
    return t ? Py_BuildValue("(idN)", st.sid, (double)st.age_ns * 1e-9, t) : nullptr;
}

// strand(sid) -> bool: ReaderHub::strand (diagnostics)
PyObject* ReaderHub_strand(ReaderHubObject* self, PyObject* arg) {
    HUB_OR_FAIL(self);
    const long sid = PyLong_AsLong(arg);
    if (sid == -1 && PyErr_Occurred()) return nullptr;
    return PyBool_FromLong(self->hub->strand((int)sid));
}

// tls_thread_ids() -> [kernel thread id] of the TLS pool's threads (placement)
PyObject* ReaderHub_tls_thread_ids(ReaderHubObject* self, PyObject*) {
    HUB_OR_FAIL(self);
    std::vector<int> ids;
    Py_BEGIN_ALLOW_THREADS
    ids = self->hub->tls_thread_ids();
    Py_END_ALLOW_THREADS
    PyObject* l = PyList_New((Py_ssize_t)ids.size());
    for (size_t i = 0; l && i < ids.size(); ++i) PyList_SET_ITEM(l, (Py_ssize_t)i, PyLong_FromLong(ids[i]));
    return l;
}

PyObject* ReaderHub_close(ReaderHubObject* self, PyObject*) {
    hub_unbind_all(self);
    if (self->hub) {
        ReaderHub* h = self->hub;
        self->hub = nullptr;
        Py_BEGIN_ALLOW_THREADS
        delete h;
        Py_END_ALLOW_THREADS
    }
    Py_RETURN_NONE;
}

PyMethodDef ReaderHub_methods[] = {
    {"fileno", (PyCFunction)ReaderHub_fileno, METH_NOARGS, "eventfd readable when take() has entries"},
    {"add", (PyCFunction)ReaderHub_add, METH_O, "add(fd) -> sid: read this socket (the hub owns and closes fd)"},
    {"add_tls", (PyCFunction)ReaderHub_add_tls, METH_VARARGS,
     "add_tls(fd, TlsContext, host, request) -> sid: handshake, write request, read decrypted (owns fd)"},
    {"error_text", (PyCFunction)ReaderHub_error_text, METH_O, "error_text(sid) -> why a stream failed ('' if not)"},
    {"remove", (PyCFunction)ReaderHub_remove, METH_O, "remove(sid): stop, close its fd, drop its queued buffers"},
    {"pause", (PyCFunction)ReaderHub_pause, METH_VARARGS, "pause(sid, paused): stop/resume reading one stream"},
    {"take", (PyCFunction)ReaderHub_take, METH_NOARGS, "take() -> [(sid, buf, view|None, read_ns, err)]"},
    {"bind", (PyCFunction)ReaderHub_bind, METH_VARARGS, "bind(sid, Pipeline, framed): take_dispatch feeds it natively"},
    {"unbind", (PyCFunction)ReaderHub_unbind, METH_O, "unbind(sid)"},
    {"take_dispatch", (PyCFunction)ReaderHub_take_dispatch, METH_NOARGS,
     "take_dispatch() -> (items needing Python, sids that had data)"},
    {"release", (PyCFunction)ReaderHub_release, METH_O, "release(buf): hand a consumed buffer back"},
    {"stats", (PyCFunction)ReaderHub_stats, METH_NOARGS, "{reads, signals, starved}"},
    {"thread_id", (PyCFunction)ReaderHub_thread_id, METH_NOARGS, "kernel thread id of the reader thread"},
    {"tls_thread_ids", (PyCFunction)ReaderHub_tls_thread_ids, METH_NOARGS, "kernel thread ids of the TLS pool"},
    {"last_read", (PyCFunction)ReaderHub_last_read, METH_O, "monotonic seconds of a stream's last read with bytes"},
    {"stream_state", (PyCFunction)ReaderHub_stream_state, METH_O, "a stream's polling state (diagnostics)"},
    {"set_stall_guard", (PyCFunction)ReaderHub_set_stall_guard, METH_O,
     "set_stall_guard(seconds): report and re-arm streams left unpolled with bytes waiting (0 = off)"},
    {"oldest_unread", (PyCFunction)ReaderHub_oldest_unread, METH_NOARGS,
     "seconds bytes have waited on a stream the hub is not polling (an upper bound), 0.0 with none"},
    {"stall_recoveries", (PyCFunction)ReaderHub_stall_recoveries, METH_NOARGS, "streams the stall guard re-armed"},
    {"last_stall", (PyCFunction)ReaderHub_last_stall, METH_NOARGS,
     "last_stall() -> (sid, seconds off, stream_state before the re-arm) | None"},
    {"strand", (PyCFunction)ReaderHub_strand, METH_O,
     "strand(sid): diagnostics — stop polling a stream as a lost wake-up would"},
    {"set_readers", (PyCFunction)ReaderHub_set_readers, METH_O, "n reader threads in all (before streams are added)"},
    {"thread_ids", (PyCFunction)ReaderHub_thread_ids, METH_NOARGS, "kernel thread ids of every reader thread"},
    {"set_depth", (PyCFunction)ReaderHub_set_depth, METH_O, "set_depth(n): read-ahead per stream in buffers (2..8)"},
    {"set_tls", (PyCFunction)ReaderHub_set_tls, METH_VARARGS,
     "set_tls(records, threads): open TLS 1.3 records in the hub, on a pool of `threads` (tls13.inc)"},
    {"close", (PyCFunction)ReaderHub_close, METH_NOARGS, "stop the thread and close every socket"},
    {nullptr, nullptr, 0, nullptr}};

PyTypeObject ReaderHubType = {PyVarObject_HEAD_INIT(nullptr, 0)};

// TlsContext(ca_pem=None, cert_pem=None, key_pem=None, verify=True): trust
// anchors from PEM (the system store without), an optional client
// certificate chain + key (mutual TLS), TLS >= 1.2.
PyObject* TlsCtx_new(PyTypeObject* type, PyObject*, PyObject*) {
    TlsCtxObject* self = (TlsCtxObject*)type->tp_alloc(type, 0);
    if (self) self->ctx = nullptr;
    return (PyObject*)self;
}

void TlsCtx_dealloc(TlsCtxObject* self) {
    if (self->ctx) SSL_CTX_free(self->ctx);
    Py_TYPE(self)->tp_free((PyObject*)self);
}

int tls_ctx_fail(const char* what) {
    PyErr_SetString(PyExc_ValueError, tls_error(what).c_str());
    return -1;
}

int TlsCtx_init(TlsCtxObject* self, PyObject* args, PyObject* kwds) {
    static const char* kwlist[] = {"ca_pem", "cert_pem", "key_pem", "verify", nullptr};
    const char *ca = nullptr, *cert = nullptr, *key = nullptr;
    Py_ssize_t can = 0, certn = 0, keyn = 0;
    int verify = 1;
    if (!PyArg_ParseTupleAndKeywords(args, kwds, "|z#z#z#p", (char**)kwlist, &ca, &can, &cert, &certn, &key, &keyn,
                                     &verify))
        return -1;
    SSL_CTX* ctx = SSL_CTX_new(TLS_client_method());
    if (!ctx) return tls_ctx_fail("context");
    if (self->ctx) SSL_CTX_free(self->ctx);
    self->ctx = ctx;
    self->verify = verify;
    SSL_CTX_set_min_proto_version(ctx, TLS1_2_VERSION);
    SSL_CTX_set_mode(ctx, SSL_MODE_ENABLE_PARTIAL_WRITE | SSL_MODE_ACCEPT_MOVING_WRITE_BUFFER);
    SSL_CTX_set_verify(ctx, verify ? SSL_VERIFY_PEER : SSL_VERIFY_NONE, nullptr);
    SSL_CTX_set_keylog_callback(ctx, tls_keylog_cb);  // the server's traffic secret (tls13.inc)
    if (ca && can) {
        BIO* bio = BIO_new_mem_buf(ca, (int)can);
        X509_STORE* store = SSL_CTX_get_cert_store(ctx);
        int added = 0;
        X509* x;
        while (bio && (x = PEM_read_bio_X509(bio, nullptr, nullptr, nullptr))) {
            if (X509_STORE_add_cert(store, x) == 1) ++added;
            X509_free(x);
        }
        BIO_free(bio);
        ERR_clear_error();  // the end of the PEM list reads as an error
        if (!added) return tls_ctx_fail("no CA certificate in ca_pem");
    } else if (SSL_CTX_set_default_verify_paths(ctx) != 1) {
        return tls_ctx_fail("system trust store");
    }
    if (cert && certn) {
        BIO* bio = BIO_new_mem_buf(cert, (int)certn);
        X509* leaf = bio ? PEM_read_bio_X509(bio, nullptr, nullptr, nullptr) : nullptr;
        if (!leaf || SSL_CTX_use_certificate(ctx, leaf) != 1) {
            if (leaf) X509_free(leaf);
            BIO_free(bio);
            return tls_ctx_fail("client certificate");
        }
        X509_free(leaf);
        X509* x;
        while ((x = PEM_read_bio_X509(bio, nullptr, nullptr, nullptr))) {
            if (SSL_CTX_add0_chain_cert(ctx, x) != 1) X509_free(x);  // add0: the context owns x
        }
        ERR_clear_error();
        BIO_free(bio);
        BIO* kb = BIO_new_mem_buf(key ? key : "", (int)keyn);
        EVP_PKEY* pk = kb ? PEM_read_bio_PrivateKey(kb, nullptr, nullptr, nullptr) : nullptr;
        BIO_free(kb);
        if (!pk || SSL_CTX_use_PrivateKey(ctx, pk) != 1) {
            if (pk) EVP_PKEY_free(pk);
            return tls_ctx_fail("client key");
        }
        EVP_PKEY_free(pk);
        if (SSL_CTX_check_private_key(ctx) != 1) return tls_ctx_fail("client key does not match the certificate");
    }
    return 0;
}

int register_readerhub(PyObject* m) {
    if (g_tls_ex < 0) g_tls_ex = SSL_get_ex_new_index(0, nullptr, nullptr, nullptr, nullptr);
    TlsCtxType.tp_name = "_kwcore.TlsContext";
    TlsCtxType.tp_basicsize = sizeof(TlsCtxObject);
    TlsCtxType.tp_flags = Py_TPFLAGS_DEFAULT;
    TlsCtxType.tp_doc = "TlsContext(ca_pem=None, cert_pem=None, key_pem=None, verify=True): watch-stream TLS";
    TlsCtxType.tp_new = TlsCtx_new;
    TlsCtxType.tp_init = (initproc)TlsCtx_init;
    TlsCtxType.tp_dealloc = (destructor)TlsCtx_dealloc;
    if (PyType_Ready(&TlsCtxType) < 0) return -1;
    Py_INCREF(&TlsCtxType);
    PyModule_AddObject(m, "TlsContext", (PyObject*)&TlsCtxType);
    ReaderHubType.tp_name = "_kwcore.ReaderHub";
    ReaderHubType.tp_basicsize = sizeof(ReaderHubObject);
    ReaderHubType.tp_flags = Py_TPFLAGS_DEFAULT;
    ReaderHubType.tp_doc = "ReaderHub(buf_bytes, nbufs, max_bytes=0): watch sockets read on a native thread";
    ReaderHubType.tp_methods = ReaderHub_methods;
    ReaderHubType.tp_new = ReaderHub_new;
    ReaderHubType.tp_init = (initproc)ReaderHub_init;
    ReaderHubType.tp_dealloc = (destructor)ReaderHub_dealloc;
    if (PyType_Ready(&ReaderHubType) < 0) return -1;
    Py_INCREF(&ReaderHubType);
    PyModule_AddObject(m, "ReaderHub", (PyObject*)&ReaderHubType);
    return 0;
}
