// engine.inc — native clusterapi notifier core + native event pipeline.
// Unity-build fragment: #included into kwcore.cpp inside its anonymous
// namespace, after the parser, decoder and response scanner it builds on.
//
// NotifierCore owns the per-connection state of the clusterapi pool
// (parallel/notifier.py documents the semantics it mirrors): request table,
// per-pod "latest seq", FIFO queues, pipelined in-flight windows, send
// buffers, response framing (scan_response), retry / supersede / give-up
// decisions and latency samples. Sockets are created and connected by
// Python (asyncio) and handed over as non-blocking fds; the event loop calls
// on_readable / on_writable. Everything per request runs here; Python only
// sees timers to schedule, fds to watch and log lines.

// (system headers are included at the top of kwcore.cpp, outside the namespace)

struct NReq {
    uint64_t seq = 0;
    std::string uid, etype, ns, name, body;
    size_t nbytes = 0;  // body bytes counted in pending_bytes (the body itself may be moved to the spool)
    int64_t read_ns = 0, sent_ns = 0;
    int64_t submit_ns = 0;  // only with keep_detail (sample_detail): when the loop submitted it
    int attempts = 0;
    int conn = 0;
};

struct NConn {
    int fd = -1;
    bool up = false;
    std::deque<uint64_t> queue, inflight;
    std::string out;
    size_t out_off = 0;
    std::string in;
    bool dirty = false;
    // TLS (https clusterapi): OpenSSL on the same non-blocking fd
    SSL* ssl = nullptr;
    bool handshaking = false;
    bool write_wants_read = false;  // SSL_write asked for readability (post-handshake messages)
    // I/O-thread mode: the thread runs this connection's syscalls, the request
    // serialisation and the response framing WITHOUT the core lock, so the
    // loop's submits never wait on a socket. Under the lock it only moves
    // requests into `stage` (queue -> in flight) and applies `resps`.
    // `io_busy` (set under the lock) marks that unlocked section: while it is
    // set the thread owns fd / ssl / out / in / stage / resps, and attach /
    // detach / give_up_all wait it out (NotifierCore::wait_idle).
    struct Staged {
        const char* p;  // the request's body: stable while it is in flight
        size_t n;
    };
    std::vector<Staged> stage;
    struct Resp {
        int status;
        bool keep;
        double retry_after;
        std::string detail;  // non-2xx only: the first 500 bytes of the body
    };
    std::vector<Resp> resps;
    bool io_busy = false;
    bool io_rd = false;      // readable (or hung up) at the last epoll_wait
    bool wblocked = false;   // the last send hit EAGAIN: wait for EPOLLOUT
    bool io_send = false;    // this round's unlocked section writes
    int io_wr = 0;           // its result: 0 done / drained, -1 would block, -2 error, -3 TLS wants read
    bool io_closed = false;  // its read saw EOF or an error
    bool io_malformed = false;
};

std::string tls_error(const char* what) {
    std::string msg = std::string("TLS ") + what;
    unsigned long e = ERR_get_error();
    if (e) {
        char buf[256];
        ERR_error_string_n(e, buf, sizeof buf);
        msg += ": ";
        msg += buf;
    }
    ERR_clear_error();
    return msg;
}

int64_t mono_ns() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (int64_t)ts.tv_sec * 1000000000LL + ts.tv_nsec;
}

// Event-loop-thread probe, off by default (one branch per call when off):
// where that thread's time goes inside the native calls, for the bench's
// bound analysis. TSC ticks, converted to ns when read (_kwcore.probe).
struct Probe {
    bool on = false;
    int64_t t0_ns = 0;
    uint64_t t0_tsc = 0;
    uint64_t calls = 0, lines = 0, bytes = 0, split = 0, wait = 0, apply = 0, run = 0, nio_calls = 0, nio = 0;
    uint64_t pump = 0;  // notifier servicing inside a batch (pl_pump), part of apply
    uint64_t tail = 0;         // partitioned batches: the loop's serial tail + tally (part of nothing else)
    uint64_t partitioned = 0;  // batches applied by partitions
    uint64_t tail_serial = 0;  // lines the partitioned batches' tail applied itself (apply_line)
    uint64_t tail_sent = 0, tail_submit = 0;  // partitioned lines the tail submitted, and the ticks it took
    uint64_t tail_rv = 0;      // ticks of the resume-point walk
    // how old the bytes are when the loop first touches them: socket read -> feed (ns x bytes)
    long double age_byte_ns = 0;
};
Probe g_probe;

// Always-on counters of the apply paths (a few relaxed adds per batch): which
// path ran and how much of it, for /metrics and the soak's record
// (_kwcore.apply_stats). Batches are applied on the event-loop thread.
struct ApplyStats {
    std::atomic<uint64_t> par_batches{0}, par_lines{0}, tail_serial{0}, tail_submits{0}, tail_lock_runs{0};
    std::atomic<uint64_t> serial_batches{0}, serial_lines{0};
    // payload cores decode built, and those its pre-filter left unbuilt (payload_prefiltered)
    std::atomic<uint64_t> payload_built{0}, payload_prefiltered{0};
};
ApplyStats g_apply;

uint32_t crc32_bytes(const char* p, size_t n) {
    // zlib's CRC-32 (what zlib.crc32 computes in Python: the same shard and
    // connection choice on both sides); table-driven per word, not per byte
    return (uint32_t)::crc32(0L, reinterpret_cast<const Bytef*>(p), (uInt)n);
}

struct NotifierCore {
    // ---- I/O thread (clusterapi.pool.io_thread). The pool's sockets are
    // registered in a private epoll served by a dedicated thread: responses are
    // read and parsed, and queued requests written, without the event loop.
    // Python (or the fused pipeline) submits under `mu` and wakes the thread;
    // the thread signals Python through an eventfd when there is something only
    // Python can act on (retry timers, logs, lost sockets, spooled records).
    std::recursive_mutex mu;
    bool threaded = false;
    int ep = -1, wake_fd = -1, py_fd = -1;
    std::thread io;
    std::atomic<bool> io_quit{false};
    std::vector<uint8_t> epout;  // EPOLLOUT registered, per connection
    int64_t signal_below = -1;   // signal Python once pending <= this (backpressure release)
    int64_t signal_below_bytes = -1;  // ... and pending_bytes <= this

    std::vector<NConn> conns;
    using ReqMap = std::unordered_map<uint64_t, NReq>;
    ReqMap reqs;
    SvMap<uint64_t> latest;  // uid -> newest seq
    SvMap<uint64_t> unsent;  // uid -> queued, unsent req (coalescing)
    // Finished requests' map nodes (and `latest` entries), kept with their
    // strings' capacity and reused by the next submits: a notification then
    // costs no allocation on the loop thread, where it was ~8 malloc/free
    // pairs (request node, uid / name / body strings, `latest` key), the
    // body's freed on the loop but allocated by a decode worker.
    std::vector<ReqMap::node_type> free_reqs;
    std::vector<SvMap<uint64_t>::node_type> free_latest;
    static constexpr size_t FREE_NODES_MAX = 4096;
    std::string head;                                  // "POST ... Content-Length: "
    int depth = 1;
    int max_attempts = 3;
    double delay = 2.0, multiplier = 2.0, max_delay = 30.0;
    bool coalesce = false, log_events = false;
    LogSink* sink = nullptr;  // per-delivery INFO lines written natively (set_log_sink), else `logs`
    std::vector<int> retryable;
    uint64_t next_seq = 0;
    std::atomic<int64_t> pending{0};  // read without the lock by Notifier_pending
    std::atomic<int64_t> pending_bytes{0};  // body bytes of those (clusterapi.pool.max_queued_bytes)
    // counter deltas since the last take()
    long long c_submitted = 0, c_delivered = 0, c_failed = 0, c_retried = 0, c_superseded = 0, c_coalesced = 0;
    long long since_pump = 0;  // submits since the last pump() (the loop's batches pump by it: pl_pump)
    long long c_retry_after = 0;  // retries delayed to the sink's Retry-After
    std::vector<int64_t> lat;  // raw event->ack samples, only with keep_samples (benchmarks)
    // Histograms kept here so the event loop does no per-notification work:
    // event->ack latency and request->ack round trip, buckets = Python's
    // metrics._BUCKETS_NS (set_histograms), read lazily via histograms().
    std::vector<int64_t> bounds;
    std::vector<uint64_t> h_lat, h_rtt;
    int64_t s_lat = 0, s_rtt = 0;
    uint64_t n_hist = 0;
    bool keep_samples = true;
    // sample_detail(True) (the bench's latency phases): per delivered request
    // (read, submit, sent, ack) in ns, so each slow notification's time splits
    // into reader->loop, the notifier's queue, and the sink round trip
    bool keep_detail = false;
    std::vector<int64_t> det;
    // clusterapi.rate_limit: one token bucket over all connections (qps <= 0: off)
    double rl_qps = 0, rl_burst = 1, rl_tokens = 0;
    int64_t rl_last = 0;
    double throttle_delay = -1;  // seconds until the next token, when a pump was throttled
    std::vector<int> throttled;

    bool take_token() {
        if (rl_qps <= 0) return true;
        const int64_t now = mono_ns();
        rl_tokens = std::min(rl_burst, rl_tokens + (double)(now - rl_last) * 1e-9 * rl_qps);
        rl_last = now;
        if (rl_tokens >= 1.0) {
            rl_tokens -= 1.0;
            return true;
        }
        const double d = (1.0 - rl_tokens) / rl_qps;
        if (throttle_delay < 0 || d < throttle_delay) throttle_delay = d;
        return false;
    }
    std::vector<std::pair<uint64_t, double>> retries;   // (seq, delay)
    std::vector<std::pair<int, std::string>> logs;      // (level, message)
    std::vector<int> dirty;
    std::vector<int> need_connect, want_write, lost;
    // Durable spool (parallel/spool.py): with spool_on, a request that fails
    // for a retryable reason after its last attempt — or is still outstanding
    // at close — is handed back to Python (`spooled`) instead of dropped.
    // spool_watch[uid] = seq of the newest *live* submit for a uid that has
    // spooled records, so a replay never overtakes newer state.
    bool spool_on = false;
    SvMap<uint64_t> spool_watch;
    std::vector<NReq> spooled;
    std::unordered_set<uint64_t> replay_seqs;  // replayed requests not yet finished
    long long c_spooled = 0;
    // TLS client context (enable_tls); nullptr = plain http
    SSL_CTX* tls = nullptr;
    std::string tls_host;
    bool tls_host_is_ip = false, tls_verify = true;

    ~NotifierCore() {
        io_end();
        for (auto& c : conns)
            if (c.ssl) SSL_free(c.ssl);
        if (tls) SSL_CTX_free(tls);
    }

    void io_wake() {
        uint64_t one = 1;
        ssize_t r = ::write(wake_fd, &one, 8);
        (void)r;
    }

    // returns the eventfd Python watches, or -1
    int io_begin() {
        if (threaded) return py_fd;
        ep = epoll_create1(EPOLL_CLOEXEC);
        wake_fd = eventfd(0, EFD_NONBLOCK | EFD_CLOEXEC);
        py_fd = eventfd(0, EFD_NONBLOCK | EFD_CLOEXEC);
        if (ep < 0 || wake_fd < 0 || py_fd < 0) return -1;
        epoll_event ev{};
        ev.events = EPOLLIN;
        ev.data.u32 = UINT32_MAX;
        epoll_ctl(ep, EPOLL_CTL_ADD, wake_fd, &ev);
        epout.assign(conns.size(), 0);
        // connections already attached (a switch from loop-driven mode): the
        // thread takes them over, writable-armed so unsent bytes go out
        for (size_t ci = 0; ci < conns.size(); ++ci)
            if (conns[ci].fd >= 0) ep_set((int)ci, EPOLL_CTL_ADD, true);
        want_write.clear();  // the loop's writers are gone; the thread arms its own
        threaded = true;
        io_quit = false;
        io = std::thread([this] { io_loop(); });
        return py_fd;
    }

    void io_end() {
        if (!threaded) return;
        io_quit = true;
        io_wake();
        if (io.joinable()) io.join();
        ::close(ep);
        ::close(wake_fd);
        ::close(py_fd);
        ep = wake_fd = py_fd = -1;
        threaded = false;
        // back to loop-driven (the sockets stay attached): requests the thread
        // staged but never serialised go into the send buffer, and connections
        // with bytes still to send need the loop's writability callback
        std::lock_guard<std::recursive_mutex> g(mu);
        for (size_t ci = 0; ci < conns.size(); ++ci) {
            NConn& c = conns[ci];
            serialise(c);
            c.wblocked = false;
            if (c.fd >= 0 && (c.out_off < c.out.size() || c.handshaking || c.write_wants_read))
                want_write.push_back((int)ci);
        }
    }

    // Python's attach / detach / give_up_all change what the I/O thread uses
    // outside the lock (the socket, the TLS session, the bodies of requests in
    // flight): wait until no connection is inside its unlocked section. That
    // section is a bounded run of non-blocking syscalls, so this is a short wait.
    // ci >= 0 waits for that connection alone (attach / detach): the thread
    // marks busy connections again every round, so waiting for all of them
    // could last many rounds under load. The waiter sleeps on idle_cv, which
    // the thread signals after each round's apply (only when someone waits).
    template <class Lock>
    void wait_idle(Lock& lk, int ci = -1) {
        if (!threaded) return;
        auto busy = [&] {
            if (ci >= 0) return (size_t)ci < conns.size() && conns[(size_t)ci].io_busy;
            for (const NConn& c : conns)
                if (c.io_busy) return true;
            return false;
        };
        while (busy()) {
            ++idle_waiters;
            idle_cv.wait(lk);
            --idle_waiters;
        }
    }
    std::condition_variable_any idle_cv;  // with mu: an unlocked section ended
    int idle_waiters = 0;                 // (mu)

    // Request heads + bodies of the staged requests into the send buffer.
    void serialise(NConn& c) {
        if (c.stage.empty()) return;
        if (c.out_off && c.out_off == c.out.size()) {
            c.out.clear();
            c.out_off = 0;
        }
        char len[24];
        for (const NConn::Staged& s : c.stage) {
            c.out.append(head);
            const int k = snprintf(len, sizeof len, "%zu\r\n\r\n", s.n);
            c.out.append(len, (size_t)k);
            c.out.append(s.p, s.n);
        }
        c.stage.clear();
    }

    void ep_set(int ci, int op, bool out) {
        epoll_event ev{};
        ev.events = EPOLLIN | EPOLLRDHUP | (out ? EPOLLOUT : 0);
        ev.data.u32 = (uint32_t)ci;
        epoll_ctl(ep, op, conns[(size_t)ci].fd, &ev);
        epout[(size_t)ci] = out;
    }

    bool has_output() const {
        return !retries.empty() || !logs.empty() || !lost.empty() || !need_connect.empty() || !spooled.empty() ||
               throttle_delay >= 0 || lat.size() >= 4096 ||
               (signal_below >= 0 && pending <= signal_below && pending_bytes <= signal_below_bytes);
    }

    // One round of the I/O thread:
    //   locked:   readiness -> per-connection flags; flush() moves queued
    //             requests into `stage` (pipeline slots, rate limit, in-flight
    //             order); pick the connections with something to do (io_busy)
    //   unlocked: serialise the staged requests, send, recv, frame responses
    //   locked:   apply the responses (delivered / failed / retry), lost
    //             connections, flush() again for the freed slots
    // The loop's submits contend only with the two locked parts, which do no
    // syscalls and no body copies.
    void io_loop() {
        epoll_event evs[64];
        std::vector<int> work;
        bool more = false;  // something is left to send: poll instead of blocking
        while (!io_quit.load()) {
            int n = epoll_wait(ep, evs, 64, more ? 0 : -1);
            if (n < 0) {
                if (errno == EINTR) continue;
                return;
            }
            work.clear();
            {
                std::lock_guard<std::recursive_mutex> g(mu);
                for (int i = 0; i < n; ++i) {
                    const uint32_t ci = evs[i].data.u32;
                    if (ci == UINT32_MAX) {
                        uint64_t v;
                        ssize_t r = ::read(wake_fd, &v, 8);
                        (void)r;
                        continue;
                    }
                    if (ci >= conns.size() || conns[ci].fd < 0) continue;  // lost since the wait
                    NConn& c = conns[ci];
                    const bool rd = evs[i].events & (EPOLLIN | EPOLLERR | EPOLLHUP | EPOLLRDHUP);
                    const bool wr = evs[i].events & EPOLLOUT;
                    if (c.handshaking) {  // rare: the TLS handshake runs under the lock
                        if (rd) on_readable((int)ci);
                        if (wr && c.fd >= 0) send_some((int)ci);
                        continue;
                    }
                    if (rd) c.io_rd = true;
                    if (wr) c.wblocked = false;
                }
                flush();  // new submits, freed pipeline slots, requeued retries
                for (size_t ci = 0; ci < conns.size(); ++ci) {
                    NConn& c = conns[ci];
                    if (c.fd < 0 || !c.up || c.handshaking) {
                        c.io_rd = false;
                        continue;
                    }
                    const bool pending_out = !c.stage.empty() || c.out_off < c.out.size();
                    c.io_send = pending_out && !c.wblocked && (!c.write_wants_read || c.io_rd);
                    if (c.io_send || c.io_rd) {
                        c.io_busy = true;
                        work.push_back((int)ci);
                    }
                }
            }
            for (int ci : work) io_unlocked(conns[(size_t)ci]);
            bool sig;
            {
                std::lock_guard<std::recursive_mutex> g(mu);
                for (int ci : work) io_apply(ci);
                if (idle_waiters && !work.empty()) idle_cv.notify_all();
                flush();
                more = false;
                for (size_t ci = 0; ci < conns.size(); ++ci) {
                    const NConn& c = conns[ci];
                    if (c.fd >= 0 && c.up && !c.handshaking && !c.wblocked && !c.write_wants_read &&
                        (!c.stage.empty() || c.out_off < c.out.size()))
                        more = true;
                }
                for (int ci : want_write)
                    if (conns[(size_t)ci].fd >= 0 && !epout[(size_t)ci]) ep_set(ci, EPOLL_CTL_MOD, true);
                want_write.clear();
                for (size_t ci = 0; ci < conns.size(); ++ci) {
                    NConn& c = conns[ci];
                    if (epout[ci] && c.fd >= 0 && !c.wblocked && !c.handshaking &&
                        (c.out_off >= c.out.size() || c.write_wants_read))
                        ep_set((int)ci, EPOLL_CTL_MOD, false);
                }
                sig = has_output();
                if (signal_below >= 0 && pending <= signal_below && pending_bytes <= signal_below_bytes)
                    signal_below = -1;
            }
            if (sig) {
                uint64_t one = 1;
                ssize_t r = ::write(py_fd, &one, 8);
                (void)r;
            }
        }
    }

    // The unlocked section (io_busy is set): only this thread touches the
    // connection's socket, TLS session and buffers, and the staged bodies
    // belong to requests in flight, which nothing frees while it runs.
    void io_unlocked(NConn& c) {
        c.io_wr = 0;
        c.io_closed = c.io_malformed = false;
        if (c.io_send) {
            c.write_wants_read = false;
            serialise(c);
            while (c.out_off < c.out.size()) {
                const ssize_t k = conn_write(c, c.out.data() + c.out_off, c.out.size() - c.out_off);
                if (k > 0) {
                    c.out_off += (size_t)k;
                    continue;
                }
                c.io_wr = k == 0 ? -2 : (int)k;
                break;
            }
            if (c.out_off == c.out.size()) {
                c.out.clear();
                c.out_off = 0;
            }
        }
        if (c.io_rd && c.io_wr != -2) {
            c.io_closed = read_in(c);
            c.io_malformed = frame_responses(c);
        }
        c.io_rd = false;
    }

    // Back under the lock: the responses framed outside it, then the
    // connection's fate.
    void io_apply(int ci) {
        NConn& c = conns[(size_t)ci];
        c.io_busy = false;
        bool must_close = c.io_malformed;
        if (must_close) logs.emplace_back(40, "Unexpected error calling clusterapi: malformed HTTP response");
        must_close |= apply_responses(c);
        if (c.io_wr == -1) {
            c.wblocked = true;
            want_write.push_back(ci);
        }
        if (c.io_wr == -2 || c.io_closed || must_close) {
            conn_lost(ci, "Connection error: Unable to connect to clusterapi");
            return;
        }
        if (c.io_wr == -3) want_write.push_back(ci);  // keep EPOLLIN: readability resumes the write
        mark(ci);
    }

    // recv / SSL_read everything available into c.in; true = closed or failed
    bool read_in(NConn& c) {
        char buf[65536];
        while (c.up) {
            ssize_t n = conn_read(c, buf, sizeof buf);
            if (n > 0) {
                c.in.append(buf, (size_t)n);
                if (!c.ssl && (size_t)n < sizeof buf) return false;  // TLS: read until WANT_READ
                continue;
            }
            return n != -1;
        }
        return false;
    }

    // Frame the complete responses in c.in into c.resps (pure: no request
    // state); true = malformed. Stops after a response that closes.
    bool frame_responses(NConn& c) {
        size_t pos = 0;
        bool bad = false;
        std::string body;
        while (pos < c.in.size()) {
            int status = 0;
            bool keep = true, until_close = false;
            double retry_after = -1.0;
            const size_t used =
                scan_response(c.in.data() + pos, c.in.size() - pos, status, keep, body, until_close, retry_after);
            if (used == 0) break;
            if (used == SIZE_MAX) {
                bad = true;
                break;
            }
            pos += used;
            if (status < 200) continue;  // interim (100, 102, 103): belongs to no request
            NConn::Resp r{status, keep, retry_after, std::string()};
            if (status < 200 || status >= 300) r.detail.assign(body, 0, 500);
            c.resps.push_back(std::move(r));
            if (!keep) break;
        }
        if (pos) c.in.erase(0, pos);
        return bad;
    }

    // Match framed responses to the in-flight requests; true = must close.
    bool apply_responses(NConn& c) {
        bool must_close = false;
        for (NConn::Resp& r : c.resps) {
            if (c.inflight.empty()) continue;  // unsolicited
            const uint64_t seq = c.inflight.front();
            c.inflight.pop_front();
            if (r.status >= 200 && r.status < 300)
                delivered(seq);
            else
                failed(seq, r.status, r.detail, r.retry_after);
            if (!r.keep) {
                must_close = true;
                break;
            }
        }
        c.resps.clear();
        return must_close;
    }

    // Start TLS on a freshly attached socket; the handshake is driven by the
    // socket's readiness (drive_handshake) before any request is written.
    bool tls_begin(int ci) {
        NConn& c = conns[(size_t)ci];
        c.ssl = SSL_new(tls);
        if (!c.ssl || SSL_set_fd(c.ssl, c.fd) != 1) {
            logs.emplace_back(40, tls_error("setup failed"));
            return false;
        }
        if (!tls_host_is_ip) SSL_set_tlsext_host_name(c.ssl, tls_host.c_str());
        if (tls_verify) {
            int ok = tls_host_is_ip ? X509_VERIFY_PARAM_set1_ip_asc(SSL_get0_param(c.ssl), tls_host.c_str())
                                    : SSL_set1_host(c.ssl, tls_host.c_str());
            if (ok != 1) {
                logs.emplace_back(40, tls_error("hostname setup failed"));
                return false;
            }
        }
        SSL_set_connect_state(c.ssl);
        c.handshaking = true;
        drive_handshake(ci);
        return true;
    }

    void drive_handshake(int ci) {
        NConn& c = conns[(size_t)ci];
        ERR_clear_error();
        int r = SSL_do_handshake(c.ssl);
        if (r == 1) {
            c.handshaking = false;
            mark(ci);  // queued requests may go now
            return;
        }
        int e = SSL_get_error(c.ssl, r);
        if (e == SSL_ERROR_WANT_READ) return;  // on_readable drives it on
        if (e == SSL_ERROR_WANT_WRITE) {
            want_write.push_back(ci);
            return;
        }
        std::string why = "Connection error: " + tls_error("handshake with clusterapi failed");
        long v = SSL_get_verify_result(c.ssl);
        if (v != X509_V_OK) why += std::string(" (") + X509_verify_cert_error_string(v) + ")";
        logs.emplace_back(40, why);
        conn_lost(ci, why);
        connect_failed(ci, why);  // like a refused connect: every queued request spends an attempt
    }

    // >0 bytes; 0 = peer closed; -1 = would block; -2 = error
    ssize_t conn_write(NConn& c, const char* p, size_t n) {
        if (!c.ssl) {
            ssize_t k = ::send(c.fd, p, n, MSG_NOSIGNAL | MSG_DONTWAIT);
            if (k >= 0) return k;
            if (errno == EAGAIN || errno == EWOULDBLOCK) return -1;
            if (errno == EINTR) return conn_write(c, p, n);
            return -2;
        }
        ERR_clear_error();
        int k = SSL_write(c.ssl, p, (int)std::min<size_t>(n, 1 << 30));
        if (k > 0) return k;
        int e = SSL_get_error(c.ssl, k);
        if (e == SSL_ERROR_WANT_WRITE) return -1;
        if (e == SSL_ERROR_WANT_READ) {
            c.write_wants_read = true;
            return -3;  // wait for readability, not writability
        }
        return -2;
    }

    ssize_t conn_read(NConn& c, char* p, size_t n) {
        if (!c.ssl) {
            ssize_t k = ::recv(c.fd, p, n, MSG_DONTWAIT);
            if (k > 0) return k;
            if (k == 0) return 0;
            if (errno == EAGAIN || errno == EWOULDBLOCK) return -1;
            if (errno == EINTR) return conn_read(c, p, n);
            return -2;
        }
        ERR_clear_error();
        int k = SSL_read(c.ssl, p, (int)n);
        if (k > 0) return k;
        int e = SSL_get_error(c.ssl, k);
        if (e == SSL_ERROR_WANT_READ || e == SSL_ERROR_WANT_WRITE) return -1;
        if (e == SSL_ERROR_ZERO_RETURN) return 0;
        return -2;
    }

    bool is_retryable(int status) const {
        if (status < 0) return true;
        for (int s : retryable)
            if (s == status) return true;
        return false;
    }

    void add_pending(int64_t n, int64_t bytes) {
        pending.fetch_add(n, std::memory_order_relaxed);
        pending_bytes.fetch_add(bytes, std::memory_order_relaxed);
    }

    void mark(int ci) {
        NConn& c = conns[(size_t)ci];
        if (!c.dirty) {
            c.dirty = true;
            dirty.push_back(ci);
        }
    }

    void set_latest(std::string_view uid, uint64_t seq) {
        auto it = latest.find(uid);
        if (it != latest.end()) {
            it->second = seq;
        } else if (!free_latest.empty()) {
            auto nh = std::move(free_latest.back());
            free_latest.pop_back();
            nh.key().assign(uid);
            nh.mapped() = seq;
            latest.insert(std::move(nh));
        } else {
            latest.emplace(std::string(uid), seq);
        }
    }
    void drop_latest(SvMap<uint64_t>::iterator it) {
        auto nh = latest.extract(it);
        if (free_latest.size() < FREE_NODES_MAX) free_latest.push_back(std::move(nh));
    }

    // body = body1 + body2 (the fused pipeline passes the payload core and
    // its tail separately: the core stays in its line job for reuse)
    // owned: the whole body, built by the caller, moved in (swapped with the
    // request's old buffer, which the caller gets back to reuse) instead of
    // copied from body1 + body2 — a ~3 KB copy per notification, read from
    // the decode worker's cache, saved on the loop thread
    void submit(std::string_view uid, std::string_view etype, std::string_view ns, std::string_view name,
                std::string_view body1, std::string_view body2, int64_t read_ns, bool replay = false,
                std::string* owned = nullptr) {
        ++c_submitted;
        ++since_pump;
        const size_t blen = owned ? owned->size() : body1.size() + body2.size();
        if (!spool_watch.empty() && !replay) {
            auto w = spool_watch.find(uid);
            if (w != spool_watch.end()) w->second = next_seq + 1;  // the seq this submit gets (or coalesces into)
        }
        if (coalesce && !replay) {
            auto it = unsent.find(uid);
            if (it != unsent.end()) {
                NReq& r = reqs[it->second];
                pending_bytes.fetch_add((int64_t)blen - (int64_t)r.nbytes, std::memory_order_relaxed);
                r.nbytes = blen;
                if (owned) {
                    r.body.swap(*owned);
                } else {
                    r.body.assign(body1);
                    r.body.append(body2);
                }
                r.etype.assign(etype);
                r.read_ns = read_ns;
                if (keep_detail) r.submit_ns = mono_ns();
                set_latest(uid, r.seq);  // same request keeps its place in the queue
                ++c_coalesced;
                return;
            }
        }
        uint64_t seq = ++next_seq;
        int ci = conns.empty() ? 0 : (int)(crc32_bytes(uid.data(), uid.size()) % conns.size());
        NReq* rp;
        if (!free_reqs.empty()) {
            auto nh = std::move(free_reqs.back());
            free_reqs.pop_back();
            nh.key() = seq;
            rp = &reqs.insert(std::move(nh)).position->second;
        } else {
            rp = &reqs[seq];
        }
        NReq& r = *rp;
        r.seq = seq;
        r.uid.assign(uid);
        r.etype.assign(etype);
        r.ns.assign(ns);
        r.name.assign(name);
        r.nbytes = blen;
        if (owned) {
            r.body.swap(*owned);
        } else {
            r.body.reserve(blen);
            r.body.assign(body1);
            r.body.append(body2);
        }
        r.read_ns = read_ns;
        r.sent_ns = 0;
        r.submit_ns = keep_detail ? mono_ns() : 0;
        r.attempts = 0;
        r.conn = ci;
        set_latest(uid, seq);
        if (coalesce && !replay) unsent[std::string(uid)] = seq;
        if (replay) replay_seqs.insert(seq);
        conns[(size_t)ci].queue.push_back(seq);
        mark(ci);
        add_pending(1, (int64_t)r.nbytes);
    }

    void delivered(uint64_t seq) {
        auto it = reqs.find(seq);
        if (it == reqs.end()) return;
        NReq& r = it->second;
        ++c_delivered;
        const int64_t now = mono_ns(), l = now - r.read_ns, rt = now - r.sent_ns;
        if (keep_samples) lat.push_back(l);
        if (keep_detail && det.size() < ((size_t)1 << 26)) {
            const int64_t q[4] = {r.read_ns, r.submit_ns, r.sent_ns, now};
            det.insert(det.end(), q, q + 4);
        }
        if (!bounds.empty()) {
            h_lat[(size_t)(std::lower_bound(bounds.begin(), bounds.end(), l) - bounds.begin())] += 1;
            h_rtt[(size_t)(std::lower_bound(bounds.begin(), bounds.end(), rt) - bounds.begin())] += 1;
            s_lat += l;
            s_rtt += rt;
            ++n_hist;
        }
        auto lt = latest.find(r.uid);
        if (lt != latest.end() && lt->second == seq) drop_latest(lt);
        if (log_events) {
            if (sink) {
                std::lock_guard<std::mutex> g(sink->mu);
                sink->begin(20);
                sink->add("Successfully notified clusterapi about ");
                sink->add(r.etype);
                sink->add(" event for ");
                sink->add(r.ns);
                sink->add("/", 1);
                sink->add(r.name);
                sink->end();
            } else {
                logs.emplace_back(20, "Successfully notified clusterapi about " + r.etype + " event for " + r.ns +
                                          "/" + r.name);
            }
        }
        finish(it);
    }

    void finish(ReqMap::iterator it) {
        if (!replay_seqs.empty()) replay_seqs.erase(it->first);
        const int64_t nb = (int64_t)it->second.nbytes;
        auto nh = reqs.extract(it);
        if (free_reqs.size() < FREE_NODES_MAX) free_reqs.push_back(std::move(nh));  // reused by submit()
        add_pending(-1, -nb);
    }

    // spoolable: the failure was transient (transport error, 5xx, 429, 408) or
    // the pool is closing — the notification is still owed to clusterapi.
    void give_up(uint64_t seq, bool spoolable = false) {
        auto it = reqs.find(seq);
        if (it == reqs.end()) return;
        NReq& r = it->second;
        auto lt = latest.find(r.uid);
        if (lt != latest.end() && lt->second == seq) drop_latest(lt);
        if (spool_on && spoolable) {
            ++c_spooled;
            spooled.push_back(std::move(r));
        } else {
            ++c_failed;
            logs.emplace_back(40, "Failed to notify clusterapi about " + r.etype + " event for " + r.ns + "/" + r.name);
        }
        finish(it);
    }

    void failed(uint64_t seq, int status, const std::string& detail, double retry_after = -1.0) {
        auto it = reqs.find(seq);
        if (it == reqs.end()) return;
        NReq& r = it->second;
        logs.emplace_back(40, status >= 0 ? "Failed to update pod data. Status: " + std::to_string(status) +
                                                ", Response: " + detail
                                          : detail);
        auto lt = latest.find(r.uid);
        if (lt == latest.end() || lt->second != seq) {
            ++c_superseded;
            finish(it);
            return;
        }
        bool transient = is_retryable(status);
        if (transient && r.attempts < max_attempts) {
            ++c_retried;
            double d = std::min(delay * std::pow(multiplier, (double)std::max(0, r.attempts - 1)), max_delay);
            if (retry_after > d) {  // the sink named its own wait (429/503): never retry sooner
                d = retry_after;
                ++c_retry_after;
            }
            retries.emplace_back(seq, d);
            return;
        }
        give_up(seq, transient);
    }

    // Python timer fired for a retry: requeue at the front unless superseded.
    void requeue(uint64_t seq, bool closing) {
        auto it = reqs.find(seq);
        if (it == reqs.end()) return;
        NReq& r = it->second;
        auto lt = latest.find(r.uid);
        if (lt == latest.end() || lt->second != seq) {
            ++c_superseded;
            finish(it);
            return;
        }
        if (closing) {
            give_up(seq, true);
            return;
        }
        conns[(size_t)r.conn].queue.push_front(seq);
        mark(r.conn);
    }

    // Move queued requests into the send buffer (up to `depth` in flight) and send.
    void pump(int ci) {
        NConn& c = conns[(size_t)ci];
        if (!c.up) {
            if (!c.queue.empty()) need_connect.push_back(ci);
            return;
        }
        if (c.handshaking) return;  // requests stay queued until TLS is up
        int64_t now = 0;
        while (!c.queue.empty() && (int)c.inflight.size() < depth) {
            uint64_t seq = c.queue.front();
            c.queue.pop_front();
            auto it = reqs.find(seq);
            if (it == reqs.end()) continue;
            if (!take_token()) {  // rate limited: stays first in line, Python re-flushes later
                c.queue.push_front(seq);
                throttled.push_back(ci);
                break;
            }
            NReq& r = it->second;
            if (coalesce) {
                auto u = unsent.find(r.uid);
                if (u != unsent.end() && u->second == seq) unsent.erase(u);
            }
            if (!now) now = mono_ns();
            r.sent_ns = now;
            r.attempts += 1;
            c.inflight.push_back(seq);
            if (threaded) {  // the I/O thread serialises it outside the lock
                c.stage.push_back({r.body.data(), r.body.size()});
                continue;
            }
            if (c.out_off && c.out_off == c.out.size()) {
                c.out.clear();
                c.out_off = 0;
            }
            c.out.append(head);
            c.out.append(std::to_string(r.body.size()));
            c.out.append("\r\n\r\n", 4);
            c.out.append(r.body);
        }
        if (!threaded) send_some(ci);
    }

    void send_some(int ci) {
        NConn& c = conns[(size_t)ci];
        if (c.handshaking) {
            drive_handshake(ci);
            return;
        }
        while (c.up && c.out_off < c.out.size()) {
            ssize_t n = conn_write(c, c.out.data() + c.out_off, c.out.size() - c.out_off);
            if (n > 0) {
                c.out_off += (size_t)n;
                continue;
            }
            if (n == -1) {
                want_write.push_back(ci);
                return;
            }
            if (n == -3) return;  // TLS wants to read first: on_readable resumes
            conn_lost(ci, "Connection error: Unable to connect to clusterapi");
            return;
        }
        if (c.out_off == c.out.size()) {
            c.out.clear();
            c.out_off = 0;
        }
    }

    void flush() {
        if (!throttled.empty()) {
            for (int ci : throttled) mark(ci);
            throttled.clear();
        }
        std::vector<int> d;
        d.swap(dirty);
        for (int ci : d) {
            conns[(size_t)ci].dirty = false;
            pump(ci);
        }
    }

    void conn_lost(int ci, const std::string& why) {
        NConn& c = conns[(size_t)ci];
        if (!c.up && c.fd < 0) return;
        if (threaded && c.fd >= 0) {
            epoll_ctl(ep, EPOLL_CTL_DEL, c.fd, nullptr);  // before Python closes the socket
            epout[(size_t)ci] = 0;
        }
        c.up = false;
        c.fd = -1;
        if (c.ssl) {
            SSL_free(c.ssl);  // the fd belongs to Python (it closes the socket)
            c.ssl = nullptr;
        }
        c.handshaking = c.write_wants_read = false;
        c.out.clear();
        c.out_off = 0;
        c.in.clear();
        c.stage.clear();  // bodies of the in-flight requests failed below
        c.resps.clear();
        c.wblocked = c.io_rd = false;
        std::deque<uint64_t> failed_now;
        failed_now.swap(c.inflight);
        lost.push_back(ci);
        for (uint64_t seq : failed_now) failed(seq, -1, why);
        if (!c.queue.empty()) need_connect.push_back(ci);
    }

    // A connect attempt failed: every queued request spends one attempt.
    void connect_failed(int ci, const std::string& why) {
        NConn& c = conns[(size_t)ci];
        std::deque<uint64_t> q;
        q.swap(c.queue);
        for (uint64_t seq : q) {
            auto it = reqs.find(seq);
            if (it != reqs.end()) it->second.attempts += 1;
            failed(seq, -1, why);
        }
    }

    // Returns false if the connection closed.
    // Service the pool from inside a long native batch (the fused pipeline
    // calls this every PUMP_LINES applied lines, on the loop thread): read the
    // responses that have arrived — freeing pipeline slots — and send what the
    // freed slots allow. Without it a batch of a few thousand events (a busy
    // watch's 4 MiB buffer, or one namespace's share of a step) holds every
    // response until it returns, and the notifications queue behind it.
    void pump() {
        since_pump = 0;
        if (threaded) return;  // the I/O thread does this continuously
        for (size_t ci = 0; ci < conns.size(); ++ci) {
            NConn& c = conns[ci];
            if (c.fd >= 0 && c.up && !c.handshaking && !c.inflight.empty()) on_readable((int)ci);
        }
        flush();
    }

    bool on_readable(int ci) {
        NConn& c = conns[(size_t)ci];
        if (c.handshaking) {
            drive_handshake(ci);
            return c.up;
        }
        if (c.write_wants_read) {
            c.write_wants_read = false;
            send_some(ci);
        }
        const bool closed = read_in(c);
        bool must_close = frame_responses(c);
        if (must_close) logs.emplace_back(40, "Unexpected error calling clusterapi: malformed HTTP response");
        must_close |= apply_responses(c);
        if (closed || must_close) {
            conn_lost(ci, "Connection error: Unable to connect to clusterapi");
            return false;
        }
        mark(ci);
        return true;
    }
};

// ----------------------------------------------------------------------------- Python type

// Every entry point takes the core's mutex: with the I/O thread running, the
// sockets are served there while Python submits, retries and reads results.
#define CORE_LOCK(self) std::lock_guard<std::recursive_mutex> core_guard_((self)->core->mu)

struct NotifierObject {
    PyObject_HEAD
    NotifierCore* core;
    PyObject* metrics;  // the Metrics.c dict (borrowed from the owner, held)
    PyObject* sink;     // _kwcore.LogSink or NULL (held: core->sink points into it)
};

void counter_add(PyObject* d, const char* key, long long delta) {
    if (!delta || !d) return;
    PyObject* k = PyUnicode_InternFromString(key);
    PyObject* cur = PyDict_GetItemWithError(d, k);
    long long v = cur ? PyLong_AsLongLong(cur) : 0;
    PyObject* nv = PyLong_FromLongLong(v + delta);
    if (nv) PyDict_SetItem(d, k, nv);
    Py_XDECREF(nv);
    Py_DECREF(k);
}

PyObject* Notifier_new(PyTypeObject* type, PyObject*, PyObject*) {
    NotifierObject* self = (NotifierObject*)type->tp_alloc(type, 0);
    if (!self) return nullptr;
    self->core = new NotifierCore();
    self->metrics = nullptr;
    self->sink = nullptr;
    return (PyObject*)self;
}

void Notifier_dealloc(NotifierObject* self) {
    delete self->core;  // joins the I/O thread before the sink can go
    Py_XDECREF(self->sink);
    Py_XDECREF(self->metrics);
    Py_TYPE(self)->tp_free((PyObject*)self);
}

int Notifier_init(NotifierObject* self, PyObject* args, PyObject* kwds) {
    static const char* kwlist[] = {"head", "connections", "depth", "max_attempts", "delay", "multiplier",
                                   "max_delay", "coalesce", "log_events", "retryable", "metrics", nullptr};
    const char* head;
    Py_ssize_t headn;
    int conns, depth, max_attempts, coalesce, log_events;
    double delay, mult, maxd;
    PyObject *retry_list, *metrics;
    if (!PyArg_ParseTupleAndKeywords(args, kwds, "y#iiidddppOO", (char**)kwlist, &head, &headn, &conns, &depth,
                                     &max_attempts, &delay, &mult, &maxd, &coalesce, &log_events, &retry_list,
                                     &metrics))
        return -1;
    NotifierCore& c = *self->core;
    c.head.assign(head, (size_t)headn);
    c.conns.assign((size_t)std::max(1, conns), NConn());
    c.depth = std::max(1, depth);
    c.max_attempts = std::max(1, max_attempts);
    c.delay = delay;
    c.multiplier = mult;
    c.max_delay = maxd;
    c.coalesce = coalesce;
    c.log_events = log_events;
    PyObject* it = PyObject_GetIter(retry_list);
    if (!it) return -1;
    PyObject* x;
    while ((x = PyIter_Next(it))) {
        c.retryable.push_back((int)PyLong_AsLong(x));
        Py_DECREF(x);
    }
    Py_DECREF(it);
    if (!PyDict_Check(metrics)) {
        PyErr_SetString(PyExc_TypeError, "metrics must be the Metrics.c dict");
        return -1;
    }
    Py_INCREF(metrics);
    Py_XSETREF(self->metrics, metrics);
    return 0;
}

bool str_arg(PyObject* o, std::string& out) {
    if (o == Py_None) {
        out = "None";
        return true;
    }
    Py_ssize_t n;
    const char* s = PyUnicode_AsUTF8AndSize(o, &n);
    if (!s) return false;
    out.assign(s, (size_t)n);
    return true;
}

// The two fields that end a notification's body, after the payload core
// without its closing brace: put together on the stack, appended once.
inline void append_body_tail(std::string& body, std::string_view ts, std::string_view etype) {
    static constexpr std::string_view a(",\"event_timestamp\":\""), b("\",\"event_type\":\""), c("\"}");
    char tail[192];  // (a timestamp is 32 bytes at most, a type this watcher sends 8)
    const size_t n = a.size() + ts.size() + b.size() + etype.size() + c.size();
    if (n > sizeof tail) {  // a caller's own type text, of any length
        body.append(a).append(ts).append(b).append(etype).append(c);
        return;
    }
    char* p = tail;
    std::memcpy(p, a.data(), a.size());
    p += a.size();
    std::memcpy(p, ts.data(), ts.size());
    p += ts.size();
    std::memcpy(p, b.data(), b.size());
    p += b.size();
    std::memcpy(p, etype.data(), etype.size());
    p += etype.size();
    std::memcpy(p, c.data(), c.size());
    body.append(tail, n);
}

// submit(uid, etype, ns, name, core: bytes, ts: str, read_ns: int)
PyObject* Notifier_submit(NotifierObject* self, PyObject* args) {
    CORE_LOCK(self);
    PyObject *uid, *et, *ns, *name;
    const char* core;
    Py_ssize_t coren;
    const char* ts;
    Py_ssize_t tsn;
    long long read_ns;
    if (!PyArg_ParseTuple(args, "OOOOy#s#L", &uid, &et, &ns, &name, &core, &coren, &ts, &tsn, &read_ns))
        return nullptr;
    std::string su, se, sn, sm;
    if (!str_arg(uid, su) || !str_arg(et, se) || !str_arg(ns, sn) || !str_arg(name, sm)) return nullptr;
    std::string tail;
    append_body_tail(tail, std::string_view(ts, (size_t)tsn), se);
    self->core->submit(su, se, sn, sm, std::string_view(core, coren > 0 ? (size_t)coren - 1 : 0), tail, read_ns);
    Py_RETURN_NONE;
}

// set_rate_limit(qps, burst): token bucket over all requests put on the wire (qps <= 0: off)
PyObject* Notifier_set_rate_limit(NotifierObject* self, PyObject* args) {
    CORE_LOCK(self);
    double qps, burst;
    if (!PyArg_ParseTuple(args, "dd", &qps, &burst)) return nullptr;
    NotifierCore& c = *self->core;
    c.rl_qps = qps;
    c.rl_burst = std::max(1.0, burst);
    c.rl_tokens = c.rl_burst;
    c.rl_last = mono_ns();
    Py_RETURN_NONE;
}

// set_histograms(bounds: [int ns], keep_samples: bool): bucket upper bounds
// (bisect_left semantics, one overflow bucket) for the native histograms
PyObject* Notifier_set_histograms(NotifierObject* self, PyObject* args) {
    CORE_LOCK(self);
    PyObject* seq;
    int keep;
    if (!PyArg_ParseTuple(args, "Op", &seq, &keep)) return nullptr;
    PyObject* fast = PySequence_Fast(seq, "bounds must be a sequence");
    if (!fast) return nullptr;
    NotifierCore& c = *self->core;
    c.bounds.clear();
    for (Py_ssize_t i = 0; i < PySequence_Fast_GET_SIZE(fast); ++i)
        c.bounds.push_back(PyLong_AsLongLong(PySequence_Fast_GET_ITEM(fast, i)));
    Py_DECREF(fast);
    if (PyErr_Occurred()) return nullptr;
    c.h_lat.assign(c.bounds.size() + 1, 0);
    c.h_rtt.assign(c.bounds.size() + 1, 0);
    c.keep_samples = keep;
    Py_RETURN_NONE;
}

// enable_tls(host, ca_file or None, verify, cert_file=None, key_file=None): https
// clusterapi. Certificates are verified against ca_file (or the system store)
// and host (DNS name or IP); cert_file/key_file present a client certificate.
PyObject* Notifier_enable_tls(NotifierObject* self, PyObject* args) {
    CORE_LOCK(self);
    const char* host;
    PyObject* ca;
    int verify;
    PyObject *cert = Py_None, *key = Py_None;
    if (!PyArg_ParseTuple(args, "sOp|OO", &host, &ca, &verify, &cert, &key)) return nullptr;
    NotifierCore& c = *self->core;
    SSL_CTX* ctx = SSL_CTX_new(TLS_client_method());
    if (!ctx) {
        PyErr_SetString(PyExc_RuntimeError, tls_error("context").c_str());
        return nullptr;
    }
    SSL_CTX_set_min_proto_version(ctx, TLS1_2_VERSION);
    SSL_CTX_set_mode(ctx, SSL_MODE_ENABLE_PARTIAL_WRITE | SSL_MODE_ACCEPT_MOVING_WRITE_BUFFER);
    if (verify) {
        SSL_CTX_set_verify(ctx, SSL_VERIFY_PEER, nullptr);
        int ok = (ca != Py_None) ? SSL_CTX_load_verify_locations(ctx, PyUnicode_AsUTF8(ca), nullptr)
                                 : SSL_CTX_set_default_verify_paths(ctx);
        if (ok != 1) {
            std::string why = tls_error("cannot load CA certificates");
            SSL_CTX_free(ctx);
            PyErr_SetString(PyExc_ValueError, why.c_str());
            return nullptr;
        }
    } else {
        SSL_CTX_set_verify(ctx, SSL_VERIFY_NONE, nullptr);
    }
    if (cert != Py_None) {  // mutual TLS
        const char* cf = PyUnicode_AsUTF8(cert);
        const char* kf = key != Py_None ? PyUnicode_AsUTF8(key) : cf;
        if (!cf || !kf || SSL_CTX_use_certificate_chain_file(ctx, cf) != 1 ||
            SSL_CTX_use_PrivateKey_file(ctx, kf, SSL_FILETYPE_PEM) != 1 || SSL_CTX_check_private_key(ctx) != 1) {
            std::string why = tls_error("cannot load the client certificate/key");
            SSL_CTX_free(ctx);
            if (!PyErr_Occurred()) PyErr_SetString(PyExc_ValueError, why.c_str());
            return nullptr;
        }
    }
    if (c.tls) SSL_CTX_free(c.tls);
    c.tls = ctx;
    c.tls_host = host;
    unsigned char addr[16];
    c.tls_host_is_ip = inet_pton(AF_INET, host, addr) == 1 || inet_pton(AF_INET6, host, addr) == 1;
    c.tls_verify = verify;
    Py_RETURN_NONE;
}

// submit_body(uid, etype, ns, name, body: bytes, read_ns) -> seq: replay of a
// spooled notification (finished body; never coalesced; tracked in replay_seqs)
PyObject* Notifier_submit_body(NotifierObject* self, PyObject* args) {
    CORE_LOCK(self);
    PyObject *uid, *et, *ns, *name;
    const char* body;
    Py_ssize_t bodyn;
    long long read_ns;
    if (!PyArg_ParseTuple(args, "OOOOy#L", &uid, &et, &ns, &name, &body, &bodyn, &read_ns)) return nullptr;
    std::string su, se, sn, sm;
    if (!str_arg(uid, su) || !str_arg(et, se) || !str_arg(ns, sn) || !str_arg(name, sm)) return nullptr;
    NotifierCore& c = *self->core;
    c.submit(su, se, sn, sm, std::string_view(body, (size_t)bodyn), std::string_view(), read_ns, true);
    return PyLong_FromUnsignedLongLong(c.next_seq);
}

// spool_control(enabled): turn spooling of owed notifications on/off
PyObject* Notifier_spool_control(NotifierObject* self, PyObject* arg) {
    CORE_LOCK(self);
    int on = PyObject_IsTrue(arg);
    if (on < 0) return nullptr;
    self->core->spool_on = on;
    Py_RETURN_NONE;
}

// spool_watch(uid, watched: bool): start/stop tracking live submits for uid
PyObject* Notifier_spool_watch(NotifierObject* self, PyObject* args) {
    CORE_LOCK(self);
    PyObject* uid;
    int on;
    if (!PyArg_ParseTuple(args, "Op", &uid, &on)) return nullptr;
    std::string su;
    if (!str_arg(uid, su)) return nullptr;
    auto& w = self->core->spool_watch;
    if (on)
        w.emplace(su, 0);
    else
        w.erase(su);
    Py_RETURN_NONE;
}

// spool_stale(uid, seq) -> True if a live notification for uid was submitted after seq
PyObject* Notifier_spool_stale(NotifierObject* self, PyObject* args) {
    CORE_LOCK(self);
    PyObject* uid;
    unsigned long long seq;
    if (!PyArg_ParseTuple(args, "OK", &uid, &seq)) return nullptr;
    std::string su;
    if (!str_arg(uid, su)) return nullptr;
    auto& w = self->core->spool_watch;
    auto it = w.find(su);
    return PyBool_FromLong(it != w.end() && it->second > seq);
}

PyObject* Notifier_replay_pending(NotifierObject* self, PyObject*) {
    CORE_LOCK(self);
    return PyLong_FromSize_t(self->core->replay_seqs.size());
}

// set_log_sink(sink or None): per-delivery INFO lines go to a _kwcore.LogSink
PyObject* Notifier_set_log_sink(NotifierObject* self, PyObject* arg);

PyObject* Notifier_flush(NotifierObject* self, PyObject*) {
    CORE_LOCK(self);
    const uint64_t p0 = g_probe.on ? __rdtsc() : 0;
    if (self->core->threaded)
        self->core->io_wake();  // the I/O thread writes
    else
        self->core->flush();
    if (p0) {
        g_probe.nio += __rdtsc() - p0;
        ++g_probe.nio_calls;
    }
    Py_RETURN_NONE;
}

PyObject* Notifier_attach(NotifierObject* self, PyObject* args) {
    int ci, fd;
    if (!PyArg_ParseTuple(args, "ii", &ci, &fd)) return nullptr;
    NotifierCore& c = *self->core;
    std::unique_lock<std::recursive_mutex> lk(c.mu);
    if (ci < 0 || (size_t)ci >= c.conns.size()) {
        PyErr_SetString(PyExc_IndexError, "connection index");
        return nullptr;
    }
    c.wait_idle(lk, ci);
    NConn& k = c.conns[(size_t)ci];
    k.fd = fd;
    k.up = true;
    k.out.clear();
    k.out_off = 0;
    k.in.clear();
    if (c.threaded) c.ep_set(ci, EPOLL_CTL_ADD, false);
    if (c.tls && !c.tls_begin(ci)) {
        c.conn_lost(ci, "Connection error: TLS setup failed");
        Py_RETURN_NONE;
    }
    c.mark(ci);
    if (c.threaded) c.io_wake();
    Py_RETURN_NONE;
}

// detach(idx, reason): the socket died or was aborted (timeout) by Python.
PyObject* Notifier_detach(NotifierObject* self, PyObject* args) {
    int ci;
    const char* why;
    if (!PyArg_ParseTuple(args, "is", &ci, &why)) return nullptr;
    NotifierCore& c = *self->core;
    std::unique_lock<std::recursive_mutex> lk(c.mu);
    if (ci < 0 || (size_t)ci >= c.conns.size()) {
        PyErr_SetString(PyExc_IndexError, "connection index");
        return nullptr;
    }
    c.wait_idle(lk, ci);  // the thread may be in recv/SSL_read on this socket: Python closes it next
    c.conn_lost(ci, why);
    Py_RETURN_NONE;
}

PyObject* Notifier_connect_failed(NotifierObject* self, PyObject* args) {
    CORE_LOCK(self);
    int ci;
    const char* why;
    if (!PyArg_ParseTuple(args, "is", &ci, &why)) return nullptr;
    self->core->connect_failed(ci, why);
    Py_RETURN_NONE;
}

PyObject* Notifier_on_readable(NotifierObject* self, PyObject* arg) {
    CORE_LOCK(self);
    int ci = (int)PyLong_AsLong(arg);
    if (ci < 0 || (size_t)ci >= self->core->conns.size()) {
        PyErr_SetString(PyExc_IndexError, "connection index");
        return nullptr;
    }
    const uint64_t p0 = g_probe.on ? __rdtsc() : 0;
    bool up = self->core->on_readable(ci);
    self->core->flush();  // refill this and any other marked connection
    if (p0) {
        g_probe.nio += __rdtsc() - p0;
        ++g_probe.nio_calls;
    }
    return PyBool_FromLong(up);
}

PyObject* Notifier_on_writable(NotifierObject* self, PyObject* arg) {
    CORE_LOCK(self);
    int ci = (int)PyLong_AsLong(arg);
    if (ci < 0 || (size_t)ci >= self->core->conns.size()) {
        PyErr_SetString(PyExc_IndexError, "connection index");
        return nullptr;
    }
    NotifierCore& c = *self->core;
    size_t before = c.want_write.size();
    const uint64_t p0 = g_probe.on ? __rdtsc() : 0;
    c.send_some(ci);
    if (p0) {
        g_probe.nio += __rdtsc() - p0;
        ++g_probe.nio_calls;
    }
    bool still = c.want_write.size() > before;
    if (still) c.want_write.pop_back();  // caller keeps the writer registered
    return PyBool_FromLong(still);
}

PyObject* Notifier_requeue(NotifierObject* self, PyObject* args) {
    CORE_LOCK(self);
    unsigned long long seq;
    int closing = 0;
    if (!PyArg_ParseTuple(args, "K|p", &seq, &closing)) return nullptr;
    self->core->requeue(seq, closing);
    if (self->core->threaded)
        self->core->io_wake();
    else
        self->core->flush();
    Py_RETURN_NONE;
}

// check_timeouts(timeout_ns) -> [idx]: connections whose oldest in-flight request is overdue
PyObject* Notifier_check_timeouts(NotifierObject* self, PyObject* arg) {
    CORE_LOCK(self);
    long long tmo = PyLong_AsLongLong(arg);
    NotifierCore& c = *self->core;
    int64_t now = mono_ns();
    PyObject* out = PyList_New(0);
    for (size_t i = 0; i < c.conns.size(); ++i) {
        NConn& k = c.conns[i];
        if (!k.up || k.inflight.empty()) continue;
        auto it = c.reqs.find(k.inflight.front());
        if (it != c.reqs.end() && now - it->second.sent_ns > tmo) {
            PyObject* v = PyLong_FromSize_t(i);
            PyList_Append(out, v);
            Py_DECREF(v);
        }
    }
    return out;
}

// take() -> (retries[(seq, delay)], logs[(level, msg)], need_connect[idx], want_write[idx], lost[idx],
//            latency samples: bytes of int64, spooled[(uid, etype, ns, name, body, seq)],
//            throttle: seconds until the rate limiter has a token again, or -1) and applies
//            counter deltas to the metrics dict.
PyObject* Notifier_take(NotifierObject* self, PyObject*) {
    CORE_LOCK(self);
    NotifierCore& c = *self->core;
    PyObject* m = self->metrics;
    counter_add(m, "notify_submitted", c.c_submitted);
    counter_add(m, "notify_delivered", c.c_delivered);
    counter_add(m, "notify_failed", c.c_failed);
    counter_add(m, "notify_retried", c.c_retried);
    counter_add(m, "notify_superseded", c.c_superseded);
    counter_add(m, "notify_coalesced", c.c_coalesced);
    counter_add(m, "notify_spooled", c.c_spooled);
    counter_add(m, "notify_retry_after_waits", c.c_retry_after);
    c.c_submitted = c.c_delivered = c.c_failed = c.c_retried = c.c_superseded = c.c_coalesced = c.c_spooled = 0;
    c.c_retry_after = 0;
    PyObject* retries = PyList_New((Py_ssize_t)c.retries.size());
    for (size_t i = 0; i < c.retries.size(); ++i)
        PyList_SET_ITEM(retries, (Py_ssize_t)i, Py_BuildValue("(Kd)", (unsigned long long)c.retries[i].first,
                                                             c.retries[i].second));
    c.retries.clear();
    PyObject* logs = PyList_New((Py_ssize_t)c.logs.size());
    for (size_t i = 0; i < c.logs.size(); ++i)
        PyList_SET_ITEM(logs, (Py_ssize_t)i, Py_BuildValue("(is#)", c.logs[i].first, c.logs[i].second.data(),
                                                          (Py_ssize_t)c.logs[i].second.size()));
    c.logs.clear();
    auto idx_list = [](std::vector<int>& v) {
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        PyObject* l = PyList_New((Py_ssize_t)v.size());
        for (size_t i = 0; i < v.size(); ++i) PyList_SET_ITEM(l, (Py_ssize_t)i, PyLong_FromLong(v[i]));
        v.clear();
        return l;
    };
    PyObject* nc = idx_list(c.need_connect);
    PyObject* ww = idx_list(c.want_write);
    PyObject* lost = idx_list(c.lost);
    PyObject* lat = PyBytes_FromStringAndSize((const char*)c.lat.data(), (Py_ssize_t)(c.lat.size() * sizeof(int64_t)));
    c.lat.clear();
    PyObject* spooled = PyList_New((Py_ssize_t)c.spooled.size());
    for (size_t i = 0; i < c.spooled.size(); ++i) {
        NReq& r = c.spooled[i];
        PyList_SET_ITEM(spooled, (Py_ssize_t)i,
                        Py_BuildValue("(s#s#s#s#y#K)", r.uid.data(), (Py_ssize_t)r.uid.size(), r.etype.data(),
                                      (Py_ssize_t)r.etype.size(), r.ns.data(), (Py_ssize_t)r.ns.size(), r.name.data(),
                                      (Py_ssize_t)r.name.size(), r.body.data(), (Py_ssize_t)r.body.size(),
                                      (unsigned long long)r.seq));
    }
    c.spooled.clear();
    double throttle = c.throttle_delay;
    c.throttle_delay = -1;
    return Py_BuildValue("(NNNNNNNd)", retries, logs, nc, ww, lost, lat, spooled, throttle);
}

// sample_detail(enable) -> bytes of int64 quadruples (read, submit, sent, ack)
// of the requests delivered since the previous call; then keeps them or not
PyObject* Notifier_sample_detail(NotifierObject* self, PyObject* arg) {
    const int on = PyObject_IsTrue(arg);
    if (on < 0) return nullptr;
    CORE_LOCK(self);
    NotifierCore& c = *self->core;
    PyObject* out = PyBytes_FromStringAndSize((const char*)c.det.data(), (Py_ssize_t)(c.det.size() * sizeof(int64_t)));
    c.det.clear();
    c.det.shrink_to_fit();
    c.keep_detail = on;
    return out;
}

// start_io() -> eventfd: serve the sockets on a dedicated thread from now on;
// Python watches the returned fd and calls take() when it is readable
PyObject* Notifier_start_io(NotifierObject* self, PyObject*) {
    CORE_LOCK(self);
    int fd = self->core->io_begin();
    if (fd < 0) return PyErr_SetFromErrno(PyExc_OSError);
    return PyLong_FromLong(fd);
}

PyObject* Notifier_stop_io(NotifierObject* self, PyObject*) {
    NotifierCore& c = *self->core;
    Py_BEGIN_ALLOW_THREADS  // the I/O thread may be waiting for `mu`: never join while holding it
    c.io_end();
    Py_END_ALLOW_THREADS
    Py_RETURN_NONE;
}

// signal_below(n, bytes=-1): ask the I/O thread to signal once pending <= n
// and pending_bytes <= bytes (backpressure release)
PyObject* Notifier_signal_below(NotifierObject* self, PyObject* args) {
    CORE_LOCK(self);
    long long n, bytes = -1;
    if (!PyArg_ParseTuple(args, "L|L", &n, &bytes)) return nullptr;
    self->core->signal_below = n;
    self->core->signal_below_bytes = bytes < 0 ? INT64_MAX : bytes;
    if (self->core->threaded) self->core->io_wake();
    Py_RETURN_NONE;
}

// histograms() -> (lat counts: bytes of uint64, lat sum, rtt counts, rtt sum, n), cumulative;
// read lazily by metrics.LatencyHistogram (no per-notification Python work)
PyObject* Notifier_histograms(NotifierObject* self, PyObject*) {
    CORE_LOCK(self);
    NotifierCore& c = *self->core;
    auto bytes = [](const std::vector<uint64_t>& v) {
        return PyBytes_FromStringAndSize((const char*)v.data(), (Py_ssize_t)(v.size() * sizeof(uint64_t)));
    };
    return Py_BuildValue("(NLNLK)", bytes(c.h_lat), (long long)c.s_lat, bytes(c.h_rtt), (long long)c.s_rtt,
                         (unsigned long long)c.n_hist);
}

PyObject* Notifier_pending(NotifierObject* self, PyObject*) {
    return PyLong_FromLongLong(self->core->pending.load(std::memory_order_relaxed));
}

// pending_in(ns) -> outstanding requests (queued, in flight or waiting to be
// retried) for pods of namespace ns: a shard handing ns over waits for this to
// reach 0 before its record goes out (engine/service.py _handover_out), so an
// old owner's retried MODIFIED cannot land after the new owner's notifications
PyObject* Notifier_pending_in(NotifierObject* self, PyObject* arg) {
    Py_ssize_t n = 0;
    const char* ns = PyUnicode_AsUTF8AndSize(arg, &n);
    if (!ns) return nullptr;
    const std::string want(ns, (size_t)n);
    long long count = 0;
    {
        CORE_LOCK(self);
        for (const auto& kv : self->core->reqs)
            if (kv.second.ns == want) ++count;
    }
    return PyLong_FromLongLong(count);
}

PyObject* Notifier_pending_bytes(NotifierObject* self, PyObject*) {
    return PyLong_FromLongLong(self->core->pending_bytes.load(std::memory_order_relaxed));
}

PyObject* Notifier_conn_state(NotifierObject* self, PyObject*) {
    CORE_LOCK(self);
    NotifierCore& c = *self->core;
    PyObject* l = PyList_New((Py_ssize_t)c.conns.size());
    for (size_t i = 0; i < c.conns.size(); ++i) {
        NConn& k = c.conns[i];
        PyList_SET_ITEM(l, (Py_ssize_t)i, Py_BuildValue("(iinn)", k.fd, (int)k.up, (Py_ssize_t)k.queue.size(),
                                                        (Py_ssize_t)k.inflight.size()));
    }
    return l;
}

// give_up_all(): on close, everything still queued or retrying fails.
PyObject* Notifier_give_up_all(NotifierObject* self, PyObject*) {
    NotifierCore& c = *self->core;
    std::unique_lock<std::recursive_mutex> lk(c.mu);
    c.wait_idle(lk);  // staged bodies belong to the requests freed here
    std::vector<uint64_t> all;
    for (auto& kv : c.reqs) all.push_back(kv.first);
    for (uint64_t s : all) c.give_up(s, true);
    for (auto& k : c.conns) {
        k.queue.clear();
        k.inflight.clear();
        k.stage.clear();
    }
    Py_RETURN_NONE;
}

PyMethodDef Notifier_methods[] = {
    {"submit", (PyCFunction)Notifier_submit, METH_VARARGS, "submit(uid, etype, ns, name, core, ts, read_ns)"},
    {"flush", (PyCFunction)Notifier_flush, METH_NOARGS, "send what can be sent"},
    {"attach", (PyCFunction)Notifier_attach, METH_VARARGS, "attach(idx, fd): a connected non-blocking socket"},
    {"detach", (PyCFunction)Notifier_detach, METH_VARARGS, "detach(idx, reason): socket lost"},
    {"connect_failed", (PyCFunction)Notifier_connect_failed, METH_VARARGS, "connect_failed(idx, reason)"},
    {"on_readable", (PyCFunction)Notifier_on_readable, METH_O, "on_readable(idx) -> still up"},
    {"on_writable", (PyCFunction)Notifier_on_writable, METH_O, "on_writable(idx) -> still wants write"},
    {"requeue", (PyCFunction)Notifier_requeue, METH_VARARGS, "requeue(seq, closing=False)"},
    {"check_timeouts", (PyCFunction)Notifier_check_timeouts, METH_O, "check_timeouts(timeout_ns) -> [idx]"},
    {"take", (PyCFunction)Notifier_take, METH_NOARGS, "take() -> (retries, logs, need_connect, want_write, lost, lat)"},
    {"pending", (PyCFunction)Notifier_pending, METH_NOARGS, "outstanding requests"},
    {"conn_state", (PyCFunction)Notifier_conn_state, METH_NOARGS, "[(fd, up, queued, inflight)]"},
    {"give_up_all", (PyCFunction)Notifier_give_up_all, METH_NOARGS, "fail (or spool) everything outstanding"},
    {"submit_body", (PyCFunction)Notifier_submit_body, METH_VARARGS,
     "submit_body(uid, etype, ns, name, body, read_ns) -> seq (spool replay)"},
    {"spool_control", (PyCFunction)Notifier_spool_control, METH_O, "spool_control(enabled)"},
    {"enable_tls", (PyCFunction)Notifier_enable_tls, METH_VARARGS,
     "enable_tls(host, ca_file, verify, cert_file=None, key_file=None)"},
    {"set_histograms", (PyCFunction)Notifier_set_histograms, METH_VARARGS, "set_histograms(bounds, keep_samples)"},
    {"set_rate_limit", (PyCFunction)Notifier_set_rate_limit, METH_VARARGS, "set_rate_limit(qps, burst)"},
    {"histograms", (PyCFunction)Notifier_histograms, METH_NOARGS, "cumulative (lat, lat_sum, rtt, rtt_sum, n)"},
    {"start_io", (PyCFunction)Notifier_start_io, METH_NOARGS, "start_io() -> eventfd (sockets served by a thread)"},
    {"stop_io", (PyCFunction)Notifier_stop_io, METH_NOARGS, "stop the I/O thread"},
    {"signal_below", (PyCFunction)Notifier_signal_below, METH_VARARGS, "signal_below(n, bytes=-1)"},
    {"pending_bytes", (PyCFunction)Notifier_pending_bytes, METH_NOARGS, "body bytes of the outstanding requests"},
    {"pending_in", (PyCFunction)Notifier_pending_in, METH_O, "pending_in(ns) -> outstanding requests for namespace ns"},
    {"spool_watch", (PyCFunction)Notifier_spool_watch, METH_VARARGS, "spool_watch(uid, watched)"},
    {"spool_stale", (PyCFunction)Notifier_spool_stale, METH_VARARGS, "spool_stale(uid, seq) -> bool"},
    {"replay_pending", (PyCFunction)Notifier_replay_pending, METH_NOARGS, "replayed requests still outstanding"},
    {"set_log_sink", (PyCFunction)Notifier_set_log_sink, METH_O, "set_log_sink(LogSink | None)"},
    {"sample_detail", (PyCFunction)Notifier_sample_detail, METH_O,
     "sample_detail(enable) -> (read, submit, sent, ack) ns per delivery since the last call"},
    {nullptr, nullptr, 0, nullptr}};

PyTypeObject NotifierType = {PyVarObject_HEAD_INIT(nullptr, 0)};

PyObject* Notifier_set_log_sink(NotifierObject* self, PyObject* arg) {
    if (arg != Py_None && !PyObject_TypeCheck(arg, &LogSinkType)) {
        PyErr_SetString(PyExc_TypeError, "set_log_sink: a _kwcore.LogSink or None");
        return nullptr;
    }
    CORE_LOCK(self);
    Py_XINCREF(arg == Py_None ? nullptr : arg);
    Py_XSETREF(self->sink, arg == Py_None ? nullptr : arg);
    self->core->sink = self->sink ? ((LogSinkObject*)self->sink)->sink : nullptr;
    Py_RETURN_NONE;
}

int register_engine(PyObject* m) {
    NotifierType.tp_name = "_kwcore.Notifier";
    NotifierType.tp_basicsize = sizeof(NotifierObject);
    NotifierType.tp_flags = Py_TPFLAGS_DEFAULT;
    NotifierType.tp_doc = "Native clusterapi notifier core (see parallel/native_notifier.py)";
    NotifierType.tp_methods = Notifier_methods;
    NotifierType.tp_new = Notifier_new;
    NotifierType.tp_init = (initproc)Notifier_init;
    NotifierType.tp_dealloc = (destructor)Notifier_dealloc;
    if (PyType_Ready(&NotifierType) < 0) return -1;
    Py_INCREF(&NotifierType);
    PyModule_AddObject(m, "Notifier", (PyObject*)&NotifierType);
    return 0;
}

// ============================================================================= native pipeline
//
// Pipeline fuses the watch decoder with EventPipeline.handle_batch
// (engine/pipeline.py, the semantic reference): chunk de-framing, NDJSON line
// splitting, single-pass field extraction, then per event the shard filter,
// the pod-cache update (the cache stays a Python dict of
// [rv, phase, ns, name, core] lists, shared with the reconcile/checkpoint
// code), the production critical filter, the per-event log line, the
// namespace filter, the phase diff, the payload core and the submit — straight
// into the native NotifierCore when one is attached. No per-event Python
// object is created except the cache's own strings.

// ----------------------------------------------------------------------------- parallel decode
//
// A feed() call is three phases: (A) de-frame and split lines (serial, the
// stream is a byte sequence), (B) decode every line into a LineJob — field
// extraction, the stateless critical filter and, for survivors, the payload
// core — which touches no Python object and runs on the DecodePool's worker
// threads plus the calling thread, and (C) apply the jobs in stream order
// under the GIL: cache, counters, stateful filters, logs, submit. Per-pod
// order is therefore exactly the serial order; (B) is where the bytes are.

// The text of a JSON string token as a view into the buffer, when it has no
// escapes (then it is the decoded text byte for byte); false otherwise.
inline bool span_view(const Span& s, std::string_view& out) {
    if (!s.is_string() || std::memchr(s.p, '\\', s.n)) return false;
    out = std::string_view(s.p + 1, s.n - 2);
    return true;
}

bool terminal_phase(const Span& s) {
    if (!s.is_string()) return false;
    const char* p = s.p + 1;
    size_t n = s.n - 2;
    // an escaped spelling of either phase is at least 11 bytes: the API's own phases never get here
    if (__builtin_expect(n >= 11 && std::memchr(p, '\\', n) != nullptr, 0)) {
        std::string text;
        json_unescape(text, p, p + n);
        return text == "Failed" || text == "Succeeded";
    }
    return (n == 6 && !std::memcmp(p, "Failed", 6)) || (n == 9 && !std::memcmp(p, "Succeeded", 9));
}

// watcher.validate
enum : uint8_t { VALIDATE_OFF = 0, VALIDATE_PAYLOAD = 1, VALIDATE_FULL = 2 };

// The texts of the namespaces the namespace filter allows, for the decode
// workers: built once by Pipeline_init and never changed, so any thread reads
// it without a lock. (The apply's verdict goes by the ids interned in
// cache->ns, a table the loop thread grows while workers decode later lines:
// no worker may touch that one.)
struct NsTextSet {
    std::unordered_set<std::string, SvHash, std::equal_to<>> texts;
    bool has(std::string_view s) const { return texts.find(s) != texts.end(); }
};

struct DecodeCfg {
    bool light, critical;
    // the payload pre-filter's inputs (payload_prefiltered): what apply_verdict
    // and other_shard decide from, as far as a line's own text decides it
    const NsTextSet* ns_texts = nullptr;  // namespace filter set: the allowed texts
    int shard_count = 1, shard_index = 0;
    bool shard_by_uid = false;
    const std::string* env_json;
    int extra = 0;  // watcher.payload_extra_fields
    uint8_t validate = VALIDATE_PAYLOAD;
    const std::string* tz_utc = nullptr;  // state_format python_repr (pyrepr.inc)
    bool failures = false;                // watcher.alerts.container_failures (findings.inc)
    const ReasonSet* reasons = nullptr;   // ... container_failure_reasons (also the extra field's)
    bool conditions = false;              // watcher.alerts.pod_conditions (findings.inc)
    const CondRules* rules = nullptr;     // ... pod_condition_rules (also the extra field's)
    bool terminating = false;             // watcher.alerts.terminating (findings.inc)
    bool deadlines = false;               // watcher.alerts.terminating_overdue_seconds > 0: a terminating line's deadline
    bool pending = false;                 // watcher.alerts.pending_overdue_seconds > 0: a Pending line's pending-since
    bool unready = false;                 // watcher.alerts.unready_overdue_seconds > 0: a Running line's unready-since
};

enum : uint8_t {
    JOB_FULL = 0,     // fields + payload (watch lines)
    JOB_FIELDS = 1,   // fields only: a LIST item before the relist compares it with the cache
    JOB_PAYLOAD = 2,  // payload only: a LIST item the comparison found changed
    JOB_SKIP = 3,     // nothing: an unchanged LIST item
};

// What the apply (apply_verdict and its two callers, apply_line and apply_par)
// reads of a decoded line, packed into two cache lines at the head of the job.
// The job is written by a decode worker on another core and read by the loop
// thread: the fields apply needs were spread over ~6 lines of LineJob (each a
// cross-core transfer); decode_line copies them here when it is done with the
// line.
struct ApplyHot {
    Span uid, ns, name, rv, phase;
    size_t uid_h = 0, ns_h = 0;  // sv_hash of the uid / namespace text (uid_hashed / ns_hashed)
    const char* err = nullptr;
    const char* payload_err = nullptr;
    int tidx = -1;
    bool status_present = false, uid_hashed = false, ns_hashed = false;
    bool has_core = false, repr_fallback = false, obj_present = false;
    bool fail_cand = false;  // container failures: the findings are non-empty (LineJob::fail_sig is their signature)
    bool cond_cand = false;  // pod conditions: likewise (LineJob::cond_sig)
    // (three bits of one byte: the struct stays two cache lines)
    bool term_cand : 1 = false;  // terminating: the pod's graceful deletion has begun (the signature itself: 1 or 0)
    bool pend_cand : 1 = false;  // pending overdue: the line has a pending-since (LineJob::pending_since)
    bool unr_cand : 1 = false;   // unready overdue: the line has an unready-since (LineJob::unready_since)
    bool pre_dropped = false;  // the critical filter kept it; the payload pre-filter left its payload unbuilt
    uint8_t part = 255;  // PodStore shard of the pod (PART_SERIAL: a line only the serial apply takes)
    uint8_t outcome = 0;  // apply_par's verdict (OUT_*), tallied and submitted by the loop thread
};

constexpr uint8_t PART_SERIAL = 255;

// hash of the key a pod without metadata.uid is cached under
inline size_t none_uid_hash() {
    static const size_t h = sv_hash(NONE_UID);
    return h;
}

static_assert(sizeof(ApplyHot) <= 128, "ApplyHot is two cache lines");

struct alignas(64) LineJob {
    ApplyHot hot;  // filled at the end of decode_line
    const char* p = nullptr;  // line bytes (the feed buffer or a stitched line)
    size_t n = 0;
    PodSpans S;
    Span type_span, obj_span;
    const char* err = nullptr;          // whole line undecodable -> INVALID
    const char* payload_err = nullptr;  // deferred sub-tree malformed -> INVALID, cache still updated
    int tidx = -1;
    bool has_core = false;
    bool bare = false;  // p..p+n is a LIST item (the pod object), not a watch line
    bool repr_fallback = false;  // python_repr: a state pyrepr.inc leaves to Python (apply_line asks it)
    bool pre_dropped = false;    // decode_payload: payload_prefiltered said so, nothing was built
    uint8_t stage = 0;  // JOB_*: what decode_line does with it (relist.inc runs two passes)
    int64_t read_ns = 0;  // socket read that brought the line (event->notify latency starts here)
    // container failures: the signature of the pod's findings, 0 for none
    // (cold: apply reads it only when hot.fail_cand says it is not 0)
    uint64_t fail_sig = 0;
    uint64_t cond_sig = 0;  // pod conditions: likewise (hot.cond_cand)
    uint64_t term_sig = 0;  // terminating: 1 or 0 (hot.term_cand says the same)
    // the deletion deadline of a terminating line (findings.inc), with
    // DecodeCfg::deadlines; cold: apply reads it only when hot.term_cand is set
    int64_t deadline = 0;
    bool has_deadline = false;
    // the pending-since of a Pending line (findings.inc), with
    // DecodeCfg::pending; cold: apply reads it only when hot.pend_cand is set
    bool has_pending = false;
    // the unready-since of a Running line (findings.inc), with
    // DecodeCfg::unready; cold: apply reads it only when hot.unr_cand is set
    bool has_unready = false;
    int64_t pending_since = 0;
    int64_t unready_since = 0;
    std::string core;
};

bool g_payload_prefilter = true;  // _kwcore.set_payload_prefilter (tests and A/B runs; not a setting)

// The payload pre-filter: will the apply drop this line for its namespace
// (OUT_NS) or its shard (OUT_SHARD) whatever the cache holds? Then nobody
// reads its payload. Decided from the line's own text and immutable
// configuration only — the same text apply_verdict's interned id and
// other_shard's crc32 stand for, so the two agree by construction. An escaped
// namespace or uid is left to the apply, which unescapes it: not decided here.
inline bool payload_prefiltered(const DecodeCfg& C, const PodSpans& S) {
    std::string_view v;
    if (C.ns_texts && span_view(S.ns, v) && !C.ns_texts->has(v)) return true;
    if (C.shard_count > 1) {
        const Span& k = C.shard_by_uid ? S.uid : S.ns;
        v = std::string_view();  // a key that is no string: "", as other_shard
        if (!k.is_string() || span_view(k, v))
            return (int)(crc32_bytes(v.data(), v.size()) % (uint32_t)C.shard_count) != C.shard_index;
    }
    return false;
}

// What decode_payload does for a line that gets a payload: the deferred
// sub-trees, their validation and the core. found / cfound: the line's
// findings where decode_payload walked them, else nullptr.
void decode_payload_core(const DecodeCfg& C, LineJob& J, const std::vector<Finding>* found,
                         const std::vector<CondFinding>* cfound) {
    PodSpans& S = J.S;
    try {
        materialize(S);  // light parse: walk spec/conditions/containerStatuses now
    } catch (const ParseError& e) {
        J.payload_err = e.msg;
        return;
    }
    if (C.validate == VALIDATE_PAYLOAD) {  // (full: the whole line passed already)
        if (const char* why = payload_spans_invalid(S)) {
            J.payload_err = why;
            return;
        }
        if (C.extra & EXTRA_FAILURES) {
            if (const char* why = findings_invalid(*found)) {
                J.payload_err = why;
                return;
            }
        }
        if (C.extra & EXTRA_CONDITIONS) {
            if (const char* why = conditions_invalid(*cfound)) {
                J.payload_err = why;
                return;
            }
        }
        if (C.extra & EXTRA_TERMINATION) {
            if (const char* why = termination_invalid(S)) {
                J.payload_err = why;
                return;
            }
        }
    }
    if (!build_core(J.core, S, *C.env_json, C.extra, C.tz_utc, found, cfound)) {
        J.repr_fallback = true;  // no GIL here: apply_line runs the Python formatter
        return;
    }
    J.core.reserve(J.core.size() + 96);  // room for the notification's tail (apply_line): no regrowth there
    J.has_core = true;
}

// The payload half of decode_line: the critical filter (stateless) and, for
// the events it keeps and the pre-filter does not drop, the deferred sub-trees
// and the payload core. prefilter false: line_core's call, for a line the
// apply wants to send after all.
void decode_payload(const DecodeCfg& C, LineJob& J, bool prefilter = true) {
    PodSpans& S = J.S;
    const int tidx = J.tidx;
    J.pre_dropped = false;
    if (tidx < T_ADDED || tidx > T_DELETED || !J.obj_span.present()) return;
    // the findings of a live pod: from the two raw status spans, before any
    // filter (stateless here; apply compares the signature with the cache's)
    static thread_local std::vector<Finding> found;
    const bool want_json = C.extra & EXTRA_FAILURES;
    J.fail_sig = 0;
    bool have_found = false;
    if ((C.failures && tidx != T_DELETED) || want_json) {
        pod_findings(S, *C.reasons, found);
        have_found = true;
        if (C.failures && tidx != T_DELETED) J.fail_sig = findings_signature(found);
    }
    // the condition findings, likewise: from the raw conditions span
    static thread_local std::vector<CondFinding> cfound;
    const bool want_cjson = C.extra & EXTRA_CONDITIONS;
    J.cond_sig = 0;
    bool have_cfound = false;
    if (__builtin_expect((C.conditions && tidx != T_DELETED) || want_cjson, 0)) {
        pod_conditions(S, *C.rules, cfound);
        have_cfound = true;
        if (C.conditions && tidx != T_DELETED) J.cond_sig = condition_signature(cfound);
    }
    // terminating: nothing to walk, both parses kept the span
    J.term_sig = C.terminating && tidx != T_DELETED ? terminating_signature(S) : 0;
    // ... and its deadline, for a terminating line only (a DELETED line never parses the timestamp)
    J.has_deadline = C.deadlines && J.term_sig && deletion_deadline(S, J.deadline);
    // pending overdue: the creation time of a live pod still Pending (three spans both parses kept)
    J.has_pending = __builtin_expect(C.pending, 0) && tidx != T_DELETED && pending_since(S, J.pending_since);
    // unready overdue: the time the Ready condition of a live Running pod turned False (walks the raw
    // conditions span, for a Running line only)
    J.has_unready = __builtin_expect(C.unready, 0) && tidx != T_DELETED && unready_since(S, J.unready_since);
    const bool candidate = (J.fail_sig | J.cond_sig | J.term_sig) != 0;  // passes the critical filter if a signature is new
    const std::vector<Finding>* fp = have_found ? &found : nullptr;
    const std::vector<CondFinding>* cp = have_cfound ? &cfound : nullptr;
    if (C.critical && !candidate && !(tidx == T_DELETED || !S.status_present || terminal_phase(S.phase))) {
        if (!J.has_pending && !J.has_unready) return;
        // A Pending line (or a Running but unready one) gets its core like a critical event, for the sweep to
        // report from (apply_commit keeps it). Nobody sends this line, so
        // whatever stands in the way of its core (the pre-filter, a malformed
        // sub-tree, a state left to the Python formatter) leaves the line as
        // the filter alone would have: nothing to report, no core.
        if (prefilter && g_payload_prefilter && payload_prefiltered(C, S)) return;
        decode_payload_core(C, J, fp, cp);
        if (!J.has_core) {
            J.payload_err = nullptr;
            J.repr_fallback = false;
        }
        return;
    }
    // (after the findings: the cache stores their signatures, sent or not)
    if (prefilter && g_payload_prefilter && payload_prefiltered(C, S)) {
        J.pre_dropped = true;
        return;
    }
    decode_payload_core(C, J, fp, cp);
}

void decode_line_impl(const DecodeCfg& C, LineJob& J) {
    if (J.stage == JOB_PAYLOAD) {  // relist pass 2: a changed item's payload
        decode_payload(C, J);
        return;
    }
    if (J.stage == JOB_SKIP) return;
    PodSpans& S = J.S;
    S.clear();
    J.type_span = J.obj_span = Span();
    J.err = J.payload_err = nullptr;
    J.has_core = J.repr_fallback = J.pre_dropped = false;
    J.fail_sig = J.cond_sig = J.term_sig = 0;
    J.has_deadline = J.has_pending = J.has_unready = false;
    J.tidx = -1;
    if (C.validate == VALIDATE_FULL) {  // json.loads' verdict on the whole line (validate.inc)
        if (const char* why = json_invalid(J.p, J.n)) {
            J.err = why;
            return;
        }
    }
    const size_t bom = has_bom(J.p, J.n) ? 3 : 0;  // as json.loads(bytes)
    if (J.bare) {  // a LIST item: the pod object itself, applied as ADDED or MODIFIED (relist.inc)
        try {
            Parser P(J.p + bom, J.p + J.n);
            if (C.light) parse_pod_light(P, S); else parse_pod(P, S);
            P.ws();
            if (P.p_ != P.end_) throw ParseError{"trailing data"};
        } catch (const ParseError& e) {
            J.err = e.msg;
            return;
        }
        J.obj_span = Span{J.p, J.n};
        J.type_span = Span();
        J.tidx = T_ADDED;  // placeholder: the relist compares with the cache before the payload pass
    } else try {
        bool not_object = false;
        Parser P(J.p + bom, J.p + J.n);
        P.object([&](const char* k, size_t kn) {
            if (KEYIS("type")) {
                J.type_span = P.value();
            } else if (KEYIS("object")) {
                S.clear();  // a repeated "object" key: the last one is the pod
                J.obj_span = Span();
                if (P.peek() != '{') {  // not an object: INVALID, unless a later "object" key is one
                    P.value();
                    not_object = true;
                    return;
                }
                not_object = false;
                const char* start = P.p_;
                if (C.light) parse_pod_light(P, S); else parse_pod(P, S);
                J.obj_span.p = start;
                J.obj_span.n = (size_t)(P.p_ - start);
            } else {
                P.value();
            }
        });
        P.ws();
        if (P.p_ != P.end_) throw ParseError{"trailing data"};
        if (not_object) throw ParseError{"object is not a JSON object"};
        J.tidx = type_index(J.type_span);
    } catch (const ParseError& e) {
        J.err = e.msg;
        return;
    }
    if (J.stage == JOB_FIELDS) return;  // relist pass 1: fields only
    decode_payload(C, J);
}

void decode_line(const DecodeCfg& C, LineJob& J) {
    decode_line_impl(C, J);
    ApplyHot& H = J.hot;
    const PodSpans& S = J.S;
    H.uid = S.uid;
    H.ns = S.ns;
    H.name = S.name;
    H.rv = S.rv;
    H.phase = S.phase;
    H.status_present = S.status_present;
    H.err = J.err;
    H.payload_err = J.payload_err;
    H.tidx = J.tidx;
    H.has_core = J.has_core;
    H.repr_fallback = J.repr_fallback;
    H.pre_dropped = J.pre_dropped;
    H.fail_cand = J.fail_sig != 0;
    H.cond_cand = J.cond_sig != 0;
    H.term_cand = J.term_sig != 0;
    H.pend_cand = J.has_pending;
    H.unr_cand = J.has_unready;
    H.obj_present = J.obj_span.present();
    // hash the lookup keys here, off the loop thread, while the line is in this core's cache
    std::string_view v;
    if ((H.uid_hashed = !J.err && span_view(S.uid, v))) H.uid_h = sv_hash(v);
    if ((H.ns_hashed = !J.err && span_view(S.ns, v))) H.ns_h = sv_hash(v);
    // the cache shard the pod lives in = the partition that applies it
    // (partitioned apply); control lines and escaped uids go to the serial apply
    H.part = PART_SERIAL;
    H.outcome = 0;
    if (!J.err && J.tidx >= T_ADDED && J.tidx <= T_DELETED && H.obj_present) {
        if (!S.uid.is_string()) H.part = (uint8_t)PodStore::shard_of(none_uid_hash());
        else if (H.uid_hashed) H.part = (uint8_t)PodStore::shard_of(H.uid_h);
    }
}

long futex_call(std::atomic<uint32_t>* w, int op, uint32_t val) {
    return syscall(SYS_futex, reinterpret_cast<uint32_t*>(w), op, val, nullptr, nullptr, 0);
}

class DecodePool {
  public:
    // Per-worker accounting, written by that worker only (relaxed): lines it
    // decoded, and how long it waited for work spinning vs asleep in the futex.
    struct alignas(64) WorkerStats {
        std::atomic<uint64_t> lines{0}, spin_ns{0}, sleep_ns{0}, sleeps{0};
        std::atomic<uint64_t> parts{0};  // partitions of a partitioned apply this worker walked
    };

    // spin_ns: how long an idle worker stays hot (pause loop) before it
    // sleeps in the futex. Hot workers pick up the next read's lines within
    // ~100 ns instead of a futex wake (~5-20 us), but burn their core
    // meanwhile — which a CPU-quota'd container pays for in throughput. The
    // caller decodes lines itself while it waits (await), so a late worker
    // costs nothing but its share: 0 (sleep at once) ran as fast as 60 us on
    // the MI355X host with ~0.9 core less per watcher
    // (profiles/decode_spin_sink_gpu_box.md).
    explicit DecodePool(int n, int64_t spin_ns = 0) : spin_ns_(spin_ns < 0 ? 0 : spin_ns) {
        // Each worker starts from the wake count at construction, not from
        // whatever it reads when the OS first runs it: a worker scheduled only
        // after start() or ~DecodePool() already bumped wake_ would otherwise
        // wait for a wake that never comes (and the destructor's join hangs).
        const uint32_t w0 = wake_.load();
        tids_.reset(new std::atomic<int>[(size_t)n]);
        stats_.reset(new WorkerStats[(size_t)n]);
        for (int i = 0; i < n; ++i) tids_[(size_t)i].store(0);
        for (int i = 0; i < n; ++i)
            threads_.emplace_back([this, w0, i] {
                tids_[(size_t)i].store((int)syscall(SYS_gettid));
                loop(w0, stats_[(size_t)i]);
            });
    }
    ~DecodePool() { stop_workers(); }
    // End and join the worker threads (WatcherService.shutdown, through
    // DecodePool.close()). The pool stays usable: with no workers the caller
    // of await()/finish() decodes every grain itself. Caller thread only,
    // between batches (no start() in flight).
    void stop_workers() {
        if (threads_.empty()) return;
        stop_.store(true);
        wake_.fetch_add(1);
        futex_call(&wake_, FUTEX_WAKE_PRIVATE, INT32_MAX);
        for (auto& t : threads_) t.join();
        threads_.clear();
    }
    int size() const { return (int)threads_.size(); }
    // kernel thread ids of the workers (for CPU pinning); 0 = not started yet
    int tid(int i) const { return tids_[(size_t)i].load(); }
    const WorkerStats& stats(int i) const { return stats_[(size_t)i]; }
    int64_t spin_ns() const { return spin_ns_; }

    // A batch whose apply phase is partitioned (engine.inc, pl_decode_apply):
    // once the decode grains are gone, every thread — workers and caller —
    // claims partitions and walks the jobs in stream order, applying the ones
    // of its partition (the pod-cache shard decode_line put in part[i]). One
    // pod's lines are all in one partition, so per-pod order is stream order.
    // Per partition, how far its walker has got, for the caller's tail that
    // runs alongside (pl_apply_partitioned): (last applied line + 1), or
    // DONE | stop once the walk is over. One cache line each: the walkers
    // write theirs every line.
    struct alignas(64) Progress {
        std::atomic<uint32_t> v{0};
    };
    static constexpr uint32_t DONE = 0x80000000u;

    struct ApplyPhase {
        bool (*apply)(void* ctx, uint32_t i);  // false: line i needs the serial path; the partition stops
        void* ctx;
        uint32_t parts;  // <= 0xFFFF
        uint32_t* stop;  // per partition: its first line not applied (n = every one)
        Progress* prog;  // per partition (optional)
    };

    // Publish jobs[0, n) to the workers. The caller then consumes them in
    // order with await(i) — applying job i while workers decode i+1.. — and
    // must call finish(n) before the jobs or their bytes go away.
    // cfgs (optional): each job's own DecodeCfg — one batch of lines from
    // several Pipelines (the reader hub's grouped dispatch); else cfg for all.
    // ap (optional): a partitioned apply phase (then the caller runs
    // apply_partitions() instead of await()).
    void start(LineJob* jobs, uint32_t n, const DecodeCfg* cfg, const DecodeCfg* const* cfgs = nullptr,
               const ApplyPhase* ap = nullptr) {
        if (n > ready_cap_) {  // no worker can touch ready_ now: the last batch is fully claimed and done
            ready_cap_ = std::max<uint32_t>(n, 2 * ready_cap_);
            ready_.reset(new std::atomic<uint32_t>[ready_cap_]);
            part_.reset(new uint8_t[ready_cap_]);
            for (uint32_t i = 0; i < ready_cap_; ++i) ready_[i].store(0, std::memory_order_relaxed);
        }
        ++gen_;
        if (gen_ == 0) ++gen_;  // 0 marks "never decoded"
        // close the cursor first: a worker still holding the previous
        // generation's cursor value can no longer claim anything, and one that
        // reads the new parameters below also sees this store (release/acquire)
        cursor_.store(((uint64_t)gen_ << 32) | CLOSED);
        done_.store(0, std::memory_order_relaxed);
        cfg_.store(cfg, std::memory_order_release);
        cfgs_.store(cfgs, std::memory_order_release);
        jobs_.store(jobs, std::memory_order_release);
        readyp_.store(ready_.get(), std::memory_order_release);
        partp_.store(part_.get(), std::memory_order_release);
        total_.store(n, std::memory_order_release);
        apply_.store(ap, std::memory_order_release);
        parts_done_.store(0, std::memory_order_relaxed);
        apply_cur_.store(ap ? ((uint64_t)gen_ << 32) | ((uint64_t)ap->parts << 16) : APPLY_CLOSED,
                         std::memory_order_release);
        cursor_.store((uint64_t)gen_ << 32, std::memory_order_release);
        wake_.fetch_add(1);
        if (sleepers_.load() > 0) futex_call(&wake_, FUTEX_WAKE_PRIVATE, INT32_MAX);
    }

    // The caller's share of a partitioned apply: claim and walk partitions
    // until none is left, then wait for the ones other threads claimed
    // (decoding unclaimed grains meanwhile). `between` runs on this thread
    // between its partitions and while it waits (the notifier's pump).
    template <class F>
    void apply_partitions(F&& between) {
        uint32_t g, p;
        while (claim_part(g, p)) {
            walk(g, p);
            between();
        }
        const ApplyPhase* ap = apply_.load(std::memory_order_acquire);
        uint32_t spins = 0;
        while (parts_done_.load(std::memory_order_acquire) < ap->parts) {
            if (!work_one()) {
                _mm_pause();
                if ((++spins & 1023) == 0) between();
            }
        }
    }

    // Block until jobs[i] is decoded; decode unclaimed grains meanwhile.
    void await(uint32_t i) {
        while (ready_[i].load(std::memory_order_acquire) != gen_)
            if (!work_one()) _mm_pause();
    }

    // jobs[i] decoded already (no waiting)
    bool ready(uint32_t i) const { return ready_[i].load(std::memory_order_acquire) == gen_; }

    // One piece of the current batch's work for a caller that is waiting on
    // it: walk an unclaimed partition, else decode a grain; false if neither
    // was left.
    bool help() {
        uint32_t g, p;
        if (claim_part(g, p)) {
            walk(g, p);
            return true;
        }
        return work_one();
    }

    void finish(uint32_t n) {
        while (done_.load(std::memory_order_acquire) < n)
            if (!work_one()) _mm_pause();
    }

  private:
    static constexpr uint32_t CLOSED = 0xFFFFFFFFu;
    static constexpr uint64_t APPLY_CLOSED = ~0ULL;
    static constexpr uint32_t GRAIN = 2;        // lines per claim (~2 x 4 KB)

    // Claim the next partition of the current generation's apply phase.
    // apply_cur_ = generation << 32 | parts << 16 | next: a claim is one CAS
    // on it, so a thread holding an older generation's value claims nothing.
    // The phase's parameters stay that generation's until every claimed
    // partition is done (the caller waits for that before the next start()).
    bool claim_part(uint32_t& g, uint32_t& p) {
        uint64_t c = apply_cur_.load(std::memory_order_acquire);
        while (true) {
            if (c == APPLY_CLOSED) return false;
            const uint32_t next = (uint32_t)(c & 0xFFFF), parts = (uint32_t)((c >> 16) & 0xFFFF);
            if (next >= parts) return false;
            if (apply_cur_.compare_exchange_weak(c, c + 1, std::memory_order_acq_rel, std::memory_order_acquire)) {
                g = (uint32_t)(c >> 32);
                p = next;
                return true;
            }
        }
    }

    // Apply partition p's lines of generation g in stream order (each waited
    // for until decoded, helping with the decode meanwhile).
    void walk(uint32_t g, uint32_t p) {
        const ApplyPhase* ap = apply_.load(std::memory_order_acquire);
        std::atomic<uint32_t>* ready = readyp_.load(std::memory_order_acquire);
        const uint8_t* part = partp_.load(std::memory_order_acquire);
        const uint32_t n = total_.load(std::memory_order_acquire);
        uint32_t i = 0;
        for (; i < n; ++i) {
            while (ready[i].load(std::memory_order_acquire) != g)
                if (!work_one()) _mm_pause();
            if (part[i] != p) continue;
            if (!ap->apply(ap->ctx, i)) break;
            if (ap->prog) ap->prog[p].v.store(i + 1, std::memory_order_release);
        }
        ap->stop[p] = i;
        if (ap->prog) ap->prog[p].v.store(DONE | i, std::memory_order_release);
        parts_done_.fetch_add(1, std::memory_order_acq_rel);
    }

    // Claim one grain of the current generation and decode it; false when
    // there is nothing left to claim. Returns the lines decoded via `got`.
    bool work_one() {
        uint32_t got;
        return work_one(got);
    }
    bool work_one(uint32_t& got) {
        got = 0;
        uint64_t c = cursor_.load(std::memory_order_acquire);
        while (true) {
            uint32_t idx = (uint32_t)c;
            if (idx == CLOSED) return false;
            const DecodeCfg* cfg = cfg_.load(std::memory_order_acquire);
            const DecodeCfg* const* cfgs = cfgs_.load(std::memory_order_acquire);
            LineJob* jobs = jobs_.load(std::memory_order_acquire);
            std::atomic<uint32_t>* ready = readyp_.load(std::memory_order_acquire);
            uint8_t* part = partp_.load(std::memory_order_acquire);
            uint32_t n = total_.load(std::memory_order_acquire);
            if (idx >= n) return false;
            uint32_t end = idx + GRAIN < n ? idx + GRAIN : n;
            uint64_t next = (c & 0xFFFFFFFF00000000ULL) | end;
            if (!cursor_.compare_exchange_weak(c, next, std::memory_order_acq_rel, std::memory_order_acquire))
                continue;  // c reloaded: another claim, or a new generation
            const uint32_t g = (uint32_t)(c >> 32);
            for (uint32_t i = idx; i < end; ++i) {
                decode_line(cfgs ? *cfgs[i] : *cfg, jobs[i]);
                part[i] = jobs[i].hot.part;
                ready[i].store(g, std::memory_order_release);
            }
            done_.fetch_add(end - idx, std::memory_order_release);
            got = end - idx;
            return true;
        }
    }

    void loop(uint32_t seen, WorkerStats& st) {
        while (true) {
            if (wake_.load() == seen) {
                const int64_t t0 = mono_ns();
                int64_t slept = 0;
                bool hot = spin_ns_ > 0;
                for (int spins = 0; wake_.load(std::memory_order_acquire) == seen; ++spins) {
                    if (hot) {
                        _mm_pause();
                        if ((spins & 255) != 255 || mono_ns() - t0 <= spin_ns_) continue;
                    }
                    hot = false;
                    const int64_t s0 = mono_ns();
                    sleepers_.fetch_add(1);
                    while (wake_.load() == seen) futex_call(&wake_, FUTEX_WAIT_PRIVATE, seen);
                    sleepers_.fetch_sub(1);
                    slept += mono_ns() - s0;
                    st.sleeps.fetch_add(1, std::memory_order_relaxed);
                }
                const int64_t waited = mono_ns() - t0;
                st.spin_ns.fetch_add((uint64_t)(waited - slept), std::memory_order_relaxed);
                st.sleep_ns.fetch_add((uint64_t)slept, std::memory_order_relaxed);
            }
            seen = wake_.load();
            if (stop_.load()) return;
            uint32_t got, lines = 0;
            while (work_one(got)) lines += got;
            if (lines) st.lines.fetch_add(lines, std::memory_order_relaxed);
            uint32_t g, p;
            while (claim_part(g, p)) {  // a partitioned apply phase: take partitions too
                walk(g, p);
                st.parts.fetch_add(1, std::memory_order_relaxed);
            }
        }
    }

    const int64_t spin_ns_;
    std::unique_ptr<WorkerStats[]> stats_;

    std::vector<std::thread> threads_;
    std::unique_ptr<std::atomic<int>[]> tids_;
    std::atomic<uint64_t> cursor_{CLOSED};
    std::atomic<uint32_t> wake_{0}, sleepers_{0}, done_{0}, total_{0};
    std::atomic<LineJob*> jobs_{nullptr};
    std::atomic<const DecodeCfg*> cfg_{nullptr};
    std::atomic<const DecodeCfg* const*> cfgs_{nullptr};
    std::atomic<std::atomic<uint32_t>*> readyp_{nullptr};
    std::atomic<uint8_t*> partp_{nullptr};
    std::atomic<const ApplyPhase*> apply_{nullptr};
    std::atomic<uint64_t> apply_cur_{APPLY_CLOSED};
    std::atomic<uint32_t> parts_done_{0};
    std::atomic<bool> stop_{false};
    // caller thread only
    uint32_t gen_ = 0;
    std::unique_ptr<std::atomic<uint32_t>[]> ready_;  // per job: generation that decoded it
    std::unique_ptr<uint8_t[]> part_;                 // per job: its partition (decode_line's hot.part)
    uint32_t ready_cap_ = 0;
};

// _kwcore.DecodePool(threads): one pool can serve several Pipelines (one per
// watch scope) because all of them are fed from the same event-loop thread.
struct DecodePoolObject {
    PyObject_HEAD
    DecodePool* pool;
};

PyObject* DecodePool_new(PyTypeObject* type, PyObject*, PyObject*) {
    DecodePoolObject* self = (DecodePoolObject*)type->tp_alloc(type, 0);
    if (self) self->pool = nullptr;
    return (PyObject*)self;
}

int DecodePool_init(DecodePoolObject* self, PyObject* args, PyObject* kwds) {
    static const char* kwlist[] = {"threads", "spin_us", nullptr};
    int n;
    double spin_us = 0.0;
    if (!PyArg_ParseTupleAndKeywords(args, kwds, "i|d", const_cast<char**>(kwlist), &n, &spin_us)) return -1;
    if (n < 1 || n > 64) {
        PyErr_SetString(PyExc_ValueError, "DecodePool threads must be in [1, 64]");
        return -1;
    }
    if (!(spin_us >= 0.0 && spin_us <= 1e6)) {
        PyErr_SetString(PyExc_ValueError, "DecodePool spin_us must be in [0, 1e6]");
        return -1;
    }
    delete self->pool;
    self->pool = new DecodePool(n, (int64_t)(spin_us * 1000.0));
    return 0;
}

// Per worker: {"lines", "spin_s", "sleep_s", "sleeps"} since the pool started.
PyObject* DecodePool_stats(DecodePoolObject* self, PyObject*) {
    const int n = self->pool ? self->pool->size() : 0;
    PyObject* out = PyList_New(n);
    if (!out) return nullptr;
    for (int i = 0; i < n; ++i) {
        const DecodePool::WorkerStats& st = self->pool->stats(i);
        PyObject* d = Py_BuildValue("{s:K,s:d,s:d,s:K,s:K}", "lines", (unsigned long long)st.lines.load(),
                                    "spin_s", (double)st.spin_ns.load() / 1e9, "sleep_s",
                                    (double)st.sleep_ns.load() / 1e9, "sleeps", (unsigned long long)st.sleeps.load(),
                                    "parts", (unsigned long long)st.parts.load());
        if (!d) {
            Py_DECREF(out);
            return nullptr;
        }
        PyList_SET_ITEM(out, i, d);
    }
    return out;
}

PyObject* DecodePool_spin_us(DecodePoolObject* self, PyObject*) {
    return PyFloat_FromDouble(self->pool ? (double)self->pool->spin_ns() / 1000.0 : 0.0);
}

void DecodePool_dealloc(DecodePoolObject* self) {
    delete self->pool;  // joins the workers (they never take the GIL)
    Py_TYPE(self)->tp_free((PyObject*)self);
}

PyObject* DecodePool_close(DecodePoolObject* self, PyObject*) {
    if (self->pool) {
        Py_BEGIN_ALLOW_THREADS  // the workers never take the GIL; joining them may take a futex wake
        self->pool->stop_workers();
        Py_END_ALLOW_THREADS
    }
    Py_RETURN_NONE;
}

PyObject* DecodePool_size(DecodePoolObject* self, PyObject*) {
    return PyLong_FromLong(self->pool ? self->pool->size() : 0);
}

PyObject* DecodePool_thread_ids(DecodePoolObject* self, PyObject*) {
    const int n = self->pool ? self->pool->size() : 0;
    PyObject* out = PyList_New(n);
    if (!out) return nullptr;
    for (int i = 0; i < n; ++i) {
        int t = 0;
        for (int spin = 0; spin < 2000 && !(t = self->pool->tid(i)); ++spin) usleep(50);  // a worker not yet scheduled
        PyList_SET_ITEM(out, i, PyLong_FromLong(t));
    }
    return out;
}

PyMethodDef DecodePool_methods[] = {
    {"size", (PyCFunction)DecodePool_size, METH_NOARGS, "worker threads"},
    {"thread_ids", (PyCFunction)DecodePool_thread_ids, METH_NOARGS, "kernel thread ids of the workers"},
    {"stats", (PyCFunction)DecodePool_stats, METH_NOARGS, "per worker: lines decoded, seconds spinning / asleep"},
    {"spin_us", (PyCFunction)DecodePool_spin_us, METH_NOARGS, "idle spin before a worker sleeps (us)"},
    {"close", (PyCFunction)DecodePool_close, METH_NOARGS,
     "end and join the worker threads (pipelines using the pool then decode on their own thread)"},
    {nullptr, nullptr, 0, nullptr}};

PyTypeObject DecodePoolType = {PyVarObject_HEAD_INIT(nullptr, 0)};

struct PipelineObject {
    PyObject_HEAD
    std::string* partial;  // the line left open by the last read (empty: none)
    ChunkState chunk;      // feed_chunked's framing state (chunked.inc), until the reader hub takes it over
    std::string* env_json;
    PodCacheObject* cache;            // _kwcore.PodCache shared with reconcile/checkpoint
    std::string* key;                 // scratch: uid text of the current event
    std::vector<uint8_t>* ns_allowed; // by namespace id (cache->ns), when nsset is set
    NsTextSet* ns_texts;              // ... the same names as texts, for decode (cfg->ns_texts); NULL without nsset
    PyObject* metrics;   // Metrics.c
    PyObject* nsset;     // frozenset or NULL
    NotifierObject* notifier;  // or NULL: submits returned to Python
    LogSinkObject* sink;       // or NULL: log lines returned to Python
    bool critical, phase_mode, log_events, log_debug, ts_utc, shard_by_uid;
    bool light;  // filters can drop events: parse filter fields first (parse_pod_light)
    int shard_count, shard_index;
    DecodeCfg* cfg;
    DecodePoolObject* pool_obj;    // NULL: decode on the calling thread only
    DecodePool* pool;              // pool_obj->pool
    std::vector<LineJob>* jobs;    // own scratch: used only when pl_run is re-entered on a thread
    std::vector<LineJob>* jobs_cur;  // this call's scratch (the thread's shared one, normally)
    size_t njobs;
    std::deque<std::string>* stitched;  // lines assembled across reads/chunks (stable addresses)
    // per-call state
    PyObject* ctrl;
    PyObject* logs;
    PyObject* submits;
    std::string* last_rv;
    bool have_rv;
    Span rv_span;  // newest resourceVersion of this call (into its buffer)
    std::string* ts;
    long long c_recv, c_crit, c_ns, c_unch, c_shard, c_bm;
    long long c_fail;  // events sent only because of watcher.alerts.container_failures
    bool failures;     // that option (cfg->failures)
    ReasonSet* reasons;
    long long c_cond;  // events sent only because of watcher.alerts.pod_conditions
    bool conditions;   // that option (cfg->conditions)
    CondRules* rules;
    long long c_term;  // events sent only because of watcher.alerts.terminating
    bool terminating;  // that option (cfg->terminating)
    bool deadlines;    // watcher.alerts.terminating_overdue_seconds > 0 (cfg->deadlines)
    bool pending;      // watcher.alerts.pending_overdue_seconds > 0 (cfg->pending)
    bool unready;      // watcher.alerts.unready_overdue_seconds > 0 (cfg->unready)
    int64_t read_ns;
    bool failed;
    bool rv_fixed;  // pl_decode_apply's partitioned path: the batch's newest resourceVersion found
    uint64_t tail_epoch;  // pl_apply_partitioned: the batch that last counted this pipeline
    // set by a Relist (relist.inc) around the lines it applies
    uint32_t relist_gen;  // nonzero: mark cache entries seen by that LIST
    bool silent;          // update the cache only (initial_list: skip)
    bool rv_known;            // last_rv holds the newest resourceVersion seen (last_rv() / set_last_rv())
    std::string* tz_utc;      // state_format python_repr (cfg->tz_utc points here)
    PyObject* repr_fallback;  // object bytes -> core bytes (models/payload.py)
};

std::string span_text(const Span& s) {
    if (!s.is_string()) return std::string();
    if (!std::memchr(s.p, '\\', s.n)) return std::string(s.p + 1, s.n - 2);
    PyObject* o = span_to_str(s);
    if (!o) {
        PyErr_Clear();
        return std::string();
    }
    Py_ssize_t n;
    const char* u = PyUnicode_AsUTF8AndSize(o, &n);
    std::string r = u ? std::string(u, (size_t)n) : std::string();
    if (!u) PyErr_Clear();
    Py_DECREF(o);
    return r;
}


// datetime.now().isoformat() (utc: datetime.now(timezone.utc).isoformat()),
// the reference's event_timestamp (pod_watcher.py:199), stamped per event as
// it is handed to the notifier. The date-time part is formatted once per second.
void event_ts(std::string& out, bool utc) {
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    static thread_local time_t cached_sec[2] = {-1, -1};
    static thread_local char cached[2][32];
    static thread_local int cached_n[2] = {0, 0};
    const int k = utc ? 1 : 0;
    if (ts.tv_sec != cached_sec[k]) {
        struct tm tmv;
        time_t secs = ts.tv_sec;
        if (utc) gmtime_r(&secs, &tmv); else localtime_r(&secs, &tmv);
        cached_n[k] = std::snprintf(cached[k], sizeof cached[k], "%04d-%02d-%02dT%02d:%02d:%02d",
                                    tmv.tm_year + 1900, tmv.tm_mon + 1, tmv.tm_mday, tmv.tm_hour, tmv.tm_min,
                                    tmv.tm_sec);
        cached_sec[k] = ts.tv_sec;
    }
    char buf[64];
    std::memcpy(buf, cached[k], (size_t)cached_n[k]);
    int n = cached_n[k];
    long micro = ts.tv_nsec / 1000;
    if (micro) {  // ".%06ld" without snprintf (this runs per notification)
        buf[n] = '.';
        for (int d = 6; d >= 1; --d) {
            buf[n + d] = (char)('0' + micro % 10);
            micro /= 10;
        }
        n += 7;
    }
    if (utc) {
        std::memcpy(buf + n, "+00:00", 6);
        n += 6;
    }
    out.assign(buf, (size_t)n);
}

void pl_log(PipelineObject* self, int level, PyObject* msg) {
    if (!msg) {
        self->failed = true;
        return;
    }
    if (!self->logs) self->logs = PyList_New(0);
    PyObject* t = Py_BuildValue("(iN)", level, msg);
    if (!t || PyList_Append(self->logs, t) < 0) self->failed = true;
    Py_XDECREF(t);
}

void pl_ctrl(PipelineObject* self, PyObject* t) {
    if (!t || PyList_Append(self->ctrl, t) < 0) self->failed = true;
    Py_XDECREF(t);
}

// ----------------------------------------------------------------------------- apply
//
// What becomes of a pod event is decided in one place (other_shard, then
// apply_verdict), written to the pod cache in one place (apply_commit),
// counted in one place (apply_tally) and handed to the native notifier in one
// place (submit_line). Two callers run them. apply_line is the serial path on
// the loop thread — also the relist's, and the fallback of a partitioned
// batch: it interns and unescapes a line's names, and around the verdict does
// what needs Python or stream order (log lines, INVALID reports, the
// python_repr fallback, the asyncio pool). apply_par is one line of one
// partition on a decode worker: it resolves names by lookup only and leaves a
// line it cannot take, untouched, to apply_line.

// What apply did with a line. OUT_NONE: nothing to count or send (a silent
// relist, a send that could not be made). A send that only an alert option
// let through the filters is OUT_SENT plus the causes: one CAUSE_* bit for
// each option whose signature was new (watcher.alerts.container_failures,
// pod_conditions, terminating), each counted in its own metric. Every value
// from OUT_SENT on is a send; the values below it carry no cause bit.
enum : uint8_t { OUT_NONE = 0, OUT_SHARD, OUT_CRIT, OUT_NS, OUT_UNCH, OUT_SENT };
enum : uint8_t { CAUSE_FAIL = 0x10, CAUSE_COND = 0x20, CAUSE_TERM = 0x40 };

// the text of g_types[tidx], for the threads that hold no GIL too
const char* const k_type_name[] = {"ADDED", "MODIFIED", "DELETED", "BOOKMARK", "ERROR", "INVALID"};

// A line's names as its caller resolved them: views of the watch buffer (of
// the serial path's scratch, for escaped text) and the interned ids. A view is
// meaningful where the field is a string (ApplyHot's span says).
struct LineNames {
    HashedView key{};  // the cache key: the uid, or none_key()
    std::string_view ns, name, rv;
    uint32_t ns_id = 0, phase_id = 0;  // 0: none
};

// the key a pod without metadata.uid is cached under
inline HashedView none_key() { return HashedView{NONE_UID, none_uid_hash()}; }

inline bool plain_text(const Span& s) { return !s.is_string() || !std::memchr(s.p + 1, '\\', s.n - 2); }
inline std::string_view str_body(const Span& s) { return std::string_view(s.p + 1, s.n - 2); }

// the views of a line whose strings are all plain: the buffer's own text (uid_h is decode_line's)
inline LineNames plain_names(const ApplyHot& S) {
    LineNames N;
    N.key = S.uid.is_string() ? HashedView{str_body(S.uid), S.uid_h} : none_key();
    if (S.ns.is_string()) N.ns = str_body(S.ns);
    if (S.name.is_string()) N.name = str_body(S.name);
    return N;  // (not rv: the loop thread's submit has no use for it, and is_string() reads the line)
}

// The shard rule (shard_count > 1): crc32 of the uid or namespace text, "" for
// none. It comes before any name is resolved — a line of another shard teaches
// the cache nothing, and its namespace need never have been seen.
inline bool other_shard(const PipelineObject* self, const ApplyHot& S, const LineNames& N) {
    const std::string_view k = !self->shard_by_uid ? N.ns : S.uid.is_string() ? N.key.s : std::string_view();
    return (int)(crc32_bytes(k.data(), k.size()) % (uint32_t)self->shard_count) != self->shard_index;
}

// the namespace filter: no set, or the interned namespace is in it
inline bool ns_kept(const PipelineObject* self, uint32_t ns_id) {
    if (!self->nsset) return true;
    const std::vector<uint8_t>& allowed = *self->ns_allowed;
    return ns_id < allowed.size() && allowed[ns_id];
}

// The verdict on a line of this shard, from the pipeline's switches, the
// line, its interned namespace and phase and the pod's cache entry as it
// stands (nullptr: unknown). Changes nothing: no Python, no lock, no
// allocation. The filters in the reference's order — critical, namespace,
// phase unchanged — and the one exception to the first and last: a line whose
// findings have a signature the cache does not hold (a new pod's is 0) passes
// them, and is then sent because of that signature alone.
inline uint8_t apply_verdict(const PipelineObject* self, const LineJob& J, uint32_t ns_id, uint32_t phase_id,
                             const CacheEntry* ent) {
    const ApplyHot& S = J.hot;
    const bool deleted = S.tidx == T_DELETED;
    // (fail_cand / cond_cand / term_cand: the signature is not 0; J's own copy is cold, read only then)
    const bool fail_event = self->failures && !deleted && S.fail_cand && J.fail_sig != (ent ? ent->sig[SIG_FAIL] : 0);
    const bool cond_event = self->conditions && !deleted && S.cond_cand && J.cond_sig != (ent ? ent->sig[SIG_COND] : 0);
    const bool term_event = self->terminating && !deleted && S.term_cand && !(ent && ent->sig[SIG_TERM]);
    const bool alert = fail_event || cond_event || term_event;
    bool only_alert = false;
    if (self->critical && !(deleted || !S.status_present || terminal_phase(S.phase))) {
        if (!alert) return OUT_CRIT;
        only_alert = true;
    }
    if (!ns_kept(self, ns_id)) return OUT_NS;
    if (self->phase_mode && !deleted && ent && ent->phase_id == phase_id) {
        if (!alert) return OUT_UNCH;
        only_alert = true;
    }
    if (!only_alert) return OUT_SENT;
    return (uint8_t)(OUT_SENT | (fail_event ? CAUSE_FAIL : 0) | (cond_event ? CAUSE_COND : 0) |
                     (term_event ? CAUSE_TERM : 0));
}

// The cache update of a line of this shard: `it` is where the verdict found
// the pod (end: unknown). DELETED erases; anything else inserts or updates the
// entry — resourceVersion, phase, the three signatures with the rest, the mark of
// the LIST being applied (relist.inc) — and a send leaves its payload core.
inline void apply_commit(PipelineObject* self, const LineJob& J, const LineNames& N, PodStore::iterator it,
                         uint8_t out) {
    const ApplyHot& S = J.hot;
    PodStore& store = *self->cache->store;
    const bool known = it != store.end();
    if (S.tidx == T_DELETED) {
        if (known) store.erase(it);
        return;
    }
    CacheEntry* ent;
    if (known) {
        ent = &it->second;
    } else {
        bool inserted;
        ent = &store.emplace(N.key, N.ns_id, inserted);
        ent->name_none = !S.name.is_string();
        if (!ent->name_none) ent->name.assign(N.name);
    }
    ent->rv_none = !S.rv.is_string();
    if (!ent->rv_none) ent->rv.assign(N.rv);
    ent->phase_id = N.phase_id;
    if (self->relist_gen) ent->list_gen = self->relist_gen;
    if (self->failures) ent->sig[SIG_FAIL] = S.fail_cand ? J.fail_sig : 0;
    if (self->conditions) ent->sig[SIG_COND] = S.cond_cand ? J.cond_sig : 0;
    if (self->terminating) ent->sig[SIG_TERM] = S.term_cand ? 1 : 0;
    // the deadline goes where the signature goes (the caller owns the entry's shard)
    if (self->deadlines && (S.term_cand || ent->timed[TIMER_DEADLINE])) {
        const bool has = S.term_cand && J.has_deadline;
        if (known) store.set_timer(TIMER_DEADLINE, it, has, J.deadline);
        else store.set_timer(TIMER_DEADLINE, *ent, has, J.deadline);
    }
    // The unready-since of a line that has none goes before the pending-since
    // is stored: the two kinds exclude each other by phase, and a line that
    // moves a pod from Running-and-unready to Pending clears the one timer, and
    // with it the old kept core, before it sets the other and keeps its own.
    const bool unready = __builtin_expect(self->unready, 0) && !self->silent;
    if (unready && !S.unr_cand && (ent->timed[TIMER_UNREADY] || ent->core_kept)) {
        if (known) store.set_timer(TIMER_UNREADY, it, false, 0); else store.set_timer(TIMER_UNREADY, *ent, false, 0);
    }
    // ... and so does the pending-since (not in a silent relist, which tracks
    // nothing); clearing it drops a kept core
    if (__builtin_expect(self->pending, 0) && !self->silent &&
        (S.pend_cand || ent->timed[TIMER_PENDING] || ent->core_kept)) {
        if (known) store.set_timer(TIMER_PENDING, it, S.pend_cand, J.pending_since);
        else store.set_timer(TIMER_PENDING, *ent, S.pend_cand, J.pending_since);
        // The core of a Pending line nobody sends, kept (and marked so) for the
        // overdue sweep: the pod has no other. Not for OUT_NS / OUT_SHARD: a pod
        // a filter drops is tracked and never reportable, as with deadlines
        // (the critical filter comes first, so OUT_CRIT has yet to ask).
        if (S.pend_cand && S.has_core && (out == OUT_UNCH || (out == OUT_CRIT && ns_kept(self, N.ns_id)))) {
            ent->core = std::make_shared<const std::string>(J.core);
            ent->core_kept = true;
        }
    }
    // ... and the unready-since of a line that has one, after the pending
    // timer went (from Pending to Running-and-unready: the reverse order);
    // its core is kept by the same rule
    if (unready && S.unr_cand) {
        if (known) store.set_timer(TIMER_UNREADY, it, true, J.unready_since);
        else store.set_timer(TIMER_UNREADY, *ent, true, J.unready_since);
        if (S.has_core && (out == OUT_UNCH || (out == OUT_CRIT && ns_kept(self, N.ns_id)))) {
            ent->core = std::make_shared<const std::string>(J.core);
            ent->core_kept = true;
        }
    }
    if (out >= OUT_SENT) {
        ent->core = std::make_shared<const std::string>(J.core);
        ent->core_kept = false;
    }
}

inline void apply_tally(PipelineObject* pl, uint8_t out) {
    switch (out) {
        case OUT_SHARD: ++pl->c_shard; break;
        case OUT_CRIT: ++pl->c_crit; break;
        case OUT_NS: ++pl->c_ns; break;
        case OUT_UNCH: ++pl->c_unch; break;
        case OUT_NONE:
        case OUT_SENT: break;
        default:  // OUT_SENT with causes: each one's metric
            if (out & CAUSE_FAIL) ++pl->c_fail;
            if (out & CAUSE_COND) ++pl->c_cond;
            if (out & CAUSE_TERM) ++pl->c_term;
            break;
    }
}

// A send to the native notifier (after apply_commit: the cache keeps the
// core as it is now). Stamped here, per event; the body is completed where
// the decode worker built it — core[:-1] + the two fields that end the
// object, in the room reserved for them — and moved into a recycled request:
// no allocation either side. The notifier's lock is recursive: the
// partitioned tail holds it over a run of these.
inline void submit_line(PipelineObject* self, LineJob& J, const LineNames& N) {
    const ApplyHot& S = J.hot;
    event_ts(*self->ts, self->ts_utc);
    const char* tname = k_type_name[S.tidx];
    J.core.pop_back();
    append_body_tail(J.core, *self->ts, tname);
    const std::string_view none("None");
    std::lock_guard<std::recursive_mutex> g(self->notifier->core->mu);
    self->notifier->core->submit(S.uid.is_string() ? N.key.s : none, tname, S.ns.is_string() ? N.ns : none,
                                 S.name.is_string() ? N.name : none, std::string_view(), std::string_view(),
                                 J.read_ns, false, &J.core);
}

// The lines that are no pod event: undecodable, without type or object, of a
// type this watcher does not know, ERROR, BOOKMARK. true: `J` was one.
bool apply_control(PipelineObject* self, const LineJob& J) {
    const ApplyHot& S = J.hot;
    const char* b = J.p;
    const size_t n = J.n;
    const int tidx = S.tidx;
    if (S.err) {
        pl_ctrl(self, make_invalid(S.err, b, n));
    } else if (tidx == -1 || !S.obj_present) {
        pl_ctrl(self, make_invalid("missing type or object", b, n));
    } else if (tidx == -2) {  // a type string this watcher does not know: handed on, as both decoders hand it on
        PyObject* t = PyTuple_New(9);
        PyObject* v[9] = {span_to_str(J.type_span), span_to_str(S.uid), span_to_str(S.ns), span_to_str(S.name),
                          span_to_str(S.rv), S.status_present ? span_to_str(S.phase) : span_to_str(Span()),
                          PyBool_FromLong(S.status_present), span_to_str(Span()), span_to_str(Span())};
        bool ok = t != nullptr;
        for (int i = 0; i < 9; ++i) {
            if (!v[i]) ok = false;
            if (t && v[i]) PyTuple_SET_ITEM(t, i, v[i]); else Py_XDECREF(v[i]);
        }
        if (!ok) {
            PyErr_Clear();
            Py_XDECREF(t);
            t = make_invalid("unknown event type", b, n);
        }
        pl_ctrl(self, t);
    } else if (tidx == T_ERROR) {
        PyObject* t = PyTuple_New(9);
        Py_INCREF(g_types[T_ERROR]);
        PyTuple_SET_ITEM(t, 0, g_types[T_ERROR]);
        for (int i = 1; i < 8; ++i) {
            PyObject* v = (i == 6) ? Py_False : Py_None;
            Py_INCREF(v);
            PyTuple_SET_ITEM(t, i, v);
        }
        PyObject* raw = PyBytes_FromStringAndSize(J.obj_span.p, (Py_ssize_t)J.obj_span.n);
        PyObject* st = raw ? PyObject_CallOneArg(g_json_loads, raw) : nullptr;
        Py_XDECREF(raw);
        if (!st) {
            PyErr_Clear();
            st = PyDict_New();
        }
        PyTuple_SET_ITEM(t, 8, st);
        pl_ctrl(self, t);
    } else if (tidx == T_BOOKMARK) {
        if (S.rv.is_string()) self->rv_span = S.rv;  // text made once per call (pl_run)
        ++self->c_bm;
    } else {
        return false;
    }
    return true;
}

// s as text: a view of the watch buffer, or of `scratch` when it is written with escapes
inline std::string_view text_of(const Span& s, std::string& scratch) {
    std::string_view v;
    if (s.is_string() && !span_view(s, v)) {
        scratch = span_text(s);
        v = scratch;
    }
    return v;
}

// A send needs its payload core: decode_line builds it for every event the
// critical filter keeps and the payload pre-filter does not drop. false: there
// is none — reported, nothing is sent.
bool line_core(PipelineObject* self, LineJob& J) {
    ApplyHot& S = J.hot;
    if (S.pre_dropped) {
        // The pre-filter dropped a line the verdict sends: they decide from the
        // same text, so this is not expected — but a send must never be lost
        // to it. The payload is built here, on the loop thread, as decode
        // would have built it.
        decode_payload(*self->cfg, J, false);
        S.payload_err = J.payload_err;
        S.has_core = J.has_core;
        S.repr_fallback = J.repr_fallback;
        S.pre_dropped = false;
    }
    if (S.payload_err) {
        // the filter fields were valid, so the cache takes this rv/phase; the
        // payload part is malformed: report the line, send nothing
        pl_ctrl(self, make_invalid(S.payload_err, J.p, J.n));
        return false;
    }
    if (S.has_core) return true;
    if (!S.repr_fallback) {
        self->failed = true;
        PyErr_SetString(PyExc_RuntimeError, "native pipeline: payload core missing");
        return false;
    }
    // python_repr: models/payload.py formats this state
    PyObject* raw = self->repr_fallback ? PyBytes_FromStringAndSize(J.obj_span.p, (Py_ssize_t)J.obj_span.n) : nullptr;
    PyObject* core = raw ? PyObject_CallOneArg(self->repr_fallback, raw) : nullptr;
    Py_XDECREF(raw);
    if (!core || !PyBytes_Check(core)) {
        PyErr_Clear();
        Py_XDECREF(core);
        pl_ctrl(self, make_invalid("container state not representable", J.p, J.n));
        return false;
    }
    J.core.assign(PyBytes_AS_STRING(core), (size_t)PyBytes_GET_SIZE(core));
    J.core.reserve(J.core.size() + 96);
    J.has_core = true;
    Py_DECREF(core);
    return true;
}

// The per-event log lines (pod_watcher.py:223 and :228): formatted and queued
// natively with a LogSink, handed back to Python without one.
void log_line(PipelineObject* self, const ApplyHot& S, const LineNames& N, uint8_t out) {
    const bool skipped = out == OUT_NS;
    if (self->sink) {
        auto who = [&](LogSink& L) {
            if (S.ns.is_string()) L.add(N.ns); else L.add("None", 4);
            L.add("/", 1);
            if (S.name.is_string()) L.add(N.name); else L.add("None", 4);
        };
        LogSink& L = *self->sink->sink;
        if (self->log_events) {
            std::lock_guard<std::mutex> g(L.mu);
            L.begin(20);
            L.add("Pod event detected: ");
            L.add(k_type_name[S.tidx]);
            L.add(" - ", 3);
            who(L);
            L.end();
        }
        if (skipped && self->log_debug) {
            std::lock_guard<std::mutex> g(L.mu);
            L.begin(10);
            L.add("Skipping pod ");
            who(L);
            L.add(" - not in target namespaces");
            L.end();
        }
        return;
    }
    if (!self->log_events && !(skipped && self->log_debug)) return;
    PyObject* nso = span_to_str(S.ns);
    PyObject* nmo = span_to_str(S.name);
    const bool ok = nso && nmo;
    if (self->log_events)
        pl_log(self, 20, ok ? PyUnicode_FromFormat("Pod event detected: %s - %S/%S", k_type_name[S.tidx], nso, nmo)
                            : nullptr);
    if (skipped && self->log_debug)
        pl_log(self, 10, ok ? PyUnicode_FromFormat("Skipping pod %S/%S - not in target namespaces", nso, nmo) : nullptr);
    Py_XDECREF(nso);
    Py_XDECREF(nmo);
}

// Phase C for one decoded line (GIL held, stream order).
void apply_line(PipelineObject* self, LineJob& J) {
    if (apply_control(self, J)) return;
    const ApplyHot& S = J.hot;  // (named S: the fields of J.S this reads, packed)
    if (!self->silent) ++self->c_recv;
    if (S.rv.is_string() && S.rv.n > 2 && !self->relist_gen) self->rv_span = S.rv;
    // Names are views of the watch buffer (escape-free strings, i.e. all of
    // them in practice); escaped text is unescaped into scratch. Text is
    // copied into the cache only on insert.
    std::string ns_buf, name_buf, rv_buf, phase_buf;
    LineNames N;
    N.key = none_key();
    if (S.uid.is_string()) {
        const std::string_view uid = text_of(S.uid, *self->key);
        N.key = HashedView{uid, S.uid_hashed ? S.uid_h : sv_hash(uid)};
    }
    N.ns = text_of(S.ns, ns_buf);
    if (self->shard_count > 1 && other_shard(self, S, N)) {
        apply_tally(self, OUT_SHARD);
        return;
    }
    N.name = text_of(S.name, name_buf);
    N.rv = text_of(S.rv, rv_buf);
    PodCacheObject* cache = self->cache;
    if (S.ns.is_string()) N.ns_id = cache->ns->intern(HashedView{N.ns, S.ns_h}, S.ns_hashed);
    if (S.status_present && S.phase.is_string()) N.phase_id = cache->phases->intern(text_of(S.phase, phase_buf));
    PodStore& store = *cache->store;
    const auto it = store.find(N.key);
    // initial_list: skip — the cache is primed, nothing is decided, counted or sent
    uint8_t out = self->silent ? OUT_NONE
                               : apply_verdict(self, J, N.ns_id, N.phase_id, it != store.end() ? &it->second : nullptr);
    // the reference logs what its critical filter keeps, before its other filters
    if (out > OUT_CRIT && (self->log_events || self->log_debug)) log_line(self, S, N, out);
    if (out >= OUT_SENT && !line_core(self, J)) out = OUT_NONE;
    apply_commit(self, J, N, it, out);
    apply_tally(self, out);
    if (out < OUT_SENT) return;
    if (self->notifier) {
        submit_line(self, J, N);
        return;
    }
    // asyncio notifier pool: hand (uid, type, ns, name, core, ts) back to Python
    event_ts(*self->ts, self->ts_utc);  // per event, at submit (not per socket read)
    PyObject* uid = span_to_str(S.uid);
    PyObject* nso = span_to_str(S.ns);
    PyObject* nmo = span_to_str(S.name);
    PyObject* core = PyBytes_FromStringAndSize(J.core.data(), (Py_ssize_t)J.core.size());
    PyObject* tso = PyUnicode_FromStringAndSize(self->ts->data(), (Py_ssize_t)self->ts->size());
    PyObject* t = (uid && nso && nmo && core && tso) ? PyTuple_Pack(6, uid, g_types[S.tidx], nso, nmo, core, tso)
                                                     : nullptr;
    Py_XDECREF(tso);
    Py_XDECREF(uid);
    Py_XDECREF(nso);
    Py_XDECREF(nmo);
    Py_XDECREF(core);
    if (!self->submits && t) self->submits = PyList_New(0);
    if (!t || !self->submits || PyList_Append(self->submits, t) < 0) self->failed = true;
    Py_XDECREF(t);
}

// ----------------------------------------------------------------------------- partitioned apply
//
// VERDICT round 3, item 3: at ~2.3M events/s the event-loop thread spent
// ~200-240 of its ~420 ns per event applying lines, in stream order. Order only
// matters per pod (the reference's unit, pod_watcher.py:266-269), and every
// line of one pod falls in one pod-cache shard (PodStore::shard_of of its
// uid hash, computed by decode_line). So a batch's apply runs as SHARDS
// partitions, claimed by the decode workers and the loop thread alike
// (DecodePool::apply_partitions): each walks the lines in stream order and
// runs the verdict and the cache update of its shard's (apply_par), with no
// Python object and no shared mutable state. The loop thread follows in
// stream order, tallies each line's outcome and submits its notification
// (apply_tally, submit_line). What needs Python or would change a table every
// partition reads (a line to report, a namespace or phase never seen, an
// escaped name, a python_repr fallback) stops that partition at that line:
// the loop thread then applies, serially and in stream order, every line a
// partition did not (apply_line). The resume point is the newest
// resourceVersion in stream order, as the serial path leaves it.

// One line of a partition (a decode worker or the loop thread; no GIL). The
// line is an ADDED/MODIFIED/DELETED event with an object and a plain uid
// (decode_line's part). false: it needs the serial path — nothing changed.
// The partitions only decide and update the cache: submitting from several
// threads made them queue on the notifier's lock behind the loop's socket
// servicing (a futex hand-off per notification).
bool apply_par(PipelineObject* self, LineJob& J) {
    ApplyHot& S = J.hot;
    if (S.payload_err) return false;  // reported by the serial path, which still updates the cache
    if (!plain_text(S.ns) || !plain_text(S.name) || !plain_text(S.rv) || !plain_text(S.phase)) return false;
    if (S.ns.is_string() && !S.ns_hashed) return false;
    LineNames N = plain_names(S);
    if (S.rv.is_string()) N.rv = str_body(S.rv);
    if (self->shard_count > 1 && other_shard(self, S, N)) {
        S.outcome = OUT_SHARD;
        return true;
    }
    PodCacheObject* cache = self->cache;
    if (S.ns.is_string() && (N.ns_id = cache->ns->lookup(HashedView{N.ns, S.ns_h}, true)) == UINT32_MAX) return false;
    if (S.status_present && S.phase.is_string() &&
        (N.phase_id = cache->phases->lookup(HashedView{str_body(S.phase), 0}, false)) == UINT32_MAX)
        return false;
    PodStore& store = *cache->store;
    const auto it = store.find(N.key);
    const uint8_t out = apply_verdict(self, J, N.ns_id, N.phase_id, it != store.end() ? &it->second : nullptr);
    if (out >= OUT_SENT && !S.has_core) return false;  // python_repr fallback / pre-dropped / no core: serial
    apply_commit(self, J, N, it, out);
    S.outcome = out;
    return true;  // tally and submit are the loop thread's, in stream order
}

struct ParCtx {
    LineJob* jobs;
    PipelineObject* const* owner;
    PipelineObject* self;
    uint32_t stop[PodStore::SHARDS];
};

bool par_apply_one(void* c, uint32_t i) {
    ParCtx& x = *static_cast<ParCtx*>(c);
    return apply_par(x.owner ? x.owner[i] : x.self, x.jobs[i]);
}

// What decode did about the payloads of a batch's lines, counted by the thread
// that applies the batch as it reaches each decoded line and added to
// ApplyStats once per batch.
struct PayloadTally {
    uint64_t built = 0, prefiltered = 0;
    void see(const ApplyHot& H) {
        built += H.has_core;
        prefiltered += H.pre_dropped;
    }
    void flush() {
        if (built) g_apply.payload_built.fetch_add(built, std::memory_order_relaxed);
        if (prefiltered) g_apply.payload_prefiltered.fetch_add(prefiltered, std::memory_order_relaxed);
        built = prefiltered = 0;
    }
};

bool g_partitioned_apply = true;       // _kwcore.set_partitioned_apply (watcher.partitioned_apply)
constexpr size_t PARTITION_MIN_LINES = 24;  // smaller batches: the fan-out costs more than it saves

// Every pipeline of the batch can take the partitioned apply: submits to the
// native notifier, no per-event log lines (their order is the stream's), not
// inside a relist, one cache for all.
bool partition_ok(PipelineObject* self, PipelineObject* const* owner, size_t nj) {
    if (!g_partitioned_apply || !self->pool || self->pool->size() == 0 || nj < PARTITION_MIN_LINES) return false;
    PipelineObject* last = nullptr;
    for (size_t i = 0; i < nj; ++i) {
        PipelineObject* pl = owner ? owner[i] : self;
        if (pl == last) continue;
        last = pl;
        if (!pl->notifier || pl->log_events || pl->log_debug || pl->relist_gen || pl->silent || pl->failed ||
            pl->cache != self->cache)
            return false;
        if (!owner) break;
    }
    return true;
}

// Phase A: split NDJSON into jobs (the chunk de-framing and the line splitter
// are chunked.inc's, shared with the reader hub's framing). Lines that end
// inside this buffer point into it; a line carried over from an earlier read
// (or chunk) is completed into `stitched`, whose elements never move.
void pl_push(PipelineObject* self, const char* b, size_t len) {
    if (!len || blank(b, len)) return;
    std::vector<LineJob>& v = *self->jobs_cur;
    if (self->njobs == v.size()) v.emplace_back();
    LineJob& J = v[self->njobs++];
    J.p = b;
    J.n = len;
    J.bare = false;
    J.stage = JOB_FULL;
    J.read_ns = self->read_ns;
}

// One piece of a line (chunked.inc's LN_* kinds, which the hub's HI_LINE /
// HI_FRAG / HI_FRAG_END are): a whole line is a job as it lies in the
// buffer, a line assembled over reads or chunks moves into `stitched` first.
inline void pl_piece(PipelineObject* self, uint8_t kind, const char* b, size_t n) {
    join_line(*self->partial, kind, b, n, [self](const char* lb, size_t ln, std::string* joined) {
        if (joined) {
            self->stitched->emplace_back(std::move(*joined));
            lb = self->stitched->back().data();
        }
        pl_push(self, lb, ln);
        return true;
    });
}

void pl_segment(PipelineObject* self, const char* data, size_t n) {
    bool open = !self->partial->empty();
    split_lines(data, 0, n, open, [&](uint8_t kind, size_t off, size_t len) {
        pl_piece(self, kind, data + off, len);
        return true;
    });
}

constexpr size_t PARALLEL_MIN_LINES = 6;  // below this a fan-out costs more than it saves
constexpr size_t PUMP_LINES = 1024;       // notifier serviced at least this often inside one batch

// Inside a batch the notifier is serviced (responses read, queued requests
// written: ~8 syscalls on four connections) once half of its pipeline window
// has been submitted since the last time, and every PUMP_LINES lines anyway.
// A fixed 256 lines pumped every ~51 notifications in production (20% of
// events notified): 70-95 ns of the loop's ~450 per line
// (profiles/decode_spin_r3_gpu_box.md); the window's half is 64 there, and
// 256 for every-event profiles (16 x 32), as before.
inline void pl_pump(PipelineObject* self, size_t i) {
    if (!self->notifier) return;
    const NotifierCore& c = *self->notifier->core;
    const long long half = std::max<long long>(8, (long long)c.conns.size() * c.depth / 2);
    if (c.since_pump >= half || i % PUMP_LINES == PUMP_LINES - 1) {
        const uint64_t t0 = g_probe.on ? __rdtsc() : 0;
        {
            std::lock_guard<std::recursive_mutex> g(self->notifier->core->mu);
            self->notifier->core->pump();
        }
        if (t0) g_probe.pump += __rdtsc() - t0;
    }
}

// Line-job scratch shared by every Pipeline fed on this thread. A watcher
// with one pod watch per namespace has one Pipeline per namespace, all fed by
// the event-loop thread; each kept its own jobs vector (up to a batch of
// LineJobs with their span vectors and ~3 KB payload cores: ~2 MB per
// namespace, ~130 MB for 64 namespace watches), cold whenever its turn came.
// Jobs live only within one pl_run call, so one vector serves them all.
struct JobScratch {
    std::vector<LineJob> jobs;
    int depth = 0;  // pl_run re-entered (never in the service): use the pipeline's own
};
thread_local JobScratch tl_jobs;

struct ScratchGuard {
    PipelineObject* self;
    explicit ScratchGuard(PipelineObject* s) : self(s) {
        self->jobs_cur = tl_jobs.depth++ == 0 ? &tl_jobs.jobs : self->jobs;
    }
    ~ScratchGuard() { --tl_jobs.depth; }
};

PyObject* pl_run_impl(PipelineObject* self, const char* data, size_t len, long long read_ns, bool framed);

// feed(data, read_ns, silent=False): `silent` applies the lines to the cache
// only, nothing is sent (a WatchList's initial DELETEDs under
// initial_list: skip — the same rule a silent Relist follows)
PyObject* pl_run(PipelineObject* self, PyObject* args, bool framed) {
    Py_buffer view;
    long long read_ns;
    int silent = 0;
    if (!PyArg_ParseTuple(args, "y*L|p", &view, &read_ns, &silent)) return nullptr;
    const bool was = self->silent;
    self->silent = was || silent;
    PyObject* res = pl_run_impl(self, (const char*)view.buf, (size_t)view.len, read_ns, framed);
    self->silent = was;
    PyBuffer_Release(&view);
    return res;
}

// Line items of a buffer the reader hub framed itself (readerhub.inc,
// HubFramer): see there.
enum : uint8_t {
    HI_LINE = LN_WHOLE,         // a whole line in this buffer
    HI_FRAG = LN_FRAG,          // bytes of a line that continues past this item
    HI_FRAG_END = LN_FRAG_END,  // the last bytes of a line begun in earlier items / buffers
    HI_DONE = 3,      // the terminating chunk and trailer: end of the body
    HI_ERROR = 4,     // bad chunk framing (HubFrame::error); nothing after it
};

struct HubItem {
    uint32_t off, len;
    uint8_t kind;
};

// One buffer's framing, written by whoever frames its bytes (the reader
// thread, or the loop's catch-up in start_framing, both under the rules in
// read_one), read by the loop after take() has handed the buffer out.
struct HubFrame {
    bool on = false;   // the buffer's bytes are framed by the hub
    size_t upto = 0;   // bytes framed so far
    std::vector<HubItem> items;
    std::string error;
};

// Phase A of one read: reset the per-call state and split `data` into line
// jobs appended to *self->jobs_cur from index self->njobs on (the caller sets
// both: a read of its own, or its place in a group batch). False: a framing
// error, whose exception is fetched into err[3] (lines before it are still
// processed, as a serial decoder would).
// Phase A of one more read in the same call (the reader hub merges
// consecutive reads of one stream into one batch): its bytes split into jobs
// after the ones already there, lines stamped with its read time.
bool pl_more(PipelineObject* self, const char* data, size_t len, long long read_ns, bool framed, PyObject* err[3]) {
    self->read_ns = read_ns;
    if (!framed) {
        pl_segment(self, data, len);
        return true;
    }
    if (self->failed) return true;
    size_t at;
    const ChunkEnd end = chunk_deframe(self->chunk, data, 0, len, at, [&](size_t off, size_t n) {
        pl_segment(self, data + off, n);
        return true;
    });
    if (end != CE_TOO_LONG && end != CE_BAD_SIZE) return true;
    set_chunk_error(self->chunk, end);
    PyErr_Fetch(&err[0], &err[1], &err[2]);
    return false;
}

bool pl_begin(PipelineObject* self, const char* data, size_t len, long long read_ns, bool framed, PyObject* err[3]) {
    self->ctrl = PyList_New(0);
    self->logs = nullptr;
    self->submits = nullptr;
    self->have_rv = false;
    self->rv_span = Span();
    self->ts->clear();
    self->c_recv = self->c_crit = self->c_ns = self->c_unch = self->c_shard = self->c_bm = self->c_fail = 0;
    self->c_cond = self->c_term = 0;
    self->read_ns = read_ns;
    self->failed = !self->ctrl;
    self->stitched->clear();
    err[0] = err[1] = err[2] = nullptr;
    return pl_more(self, data, len, read_ns, framed, err);
}

bool pl_items(PipelineObject* self, const char* data, const HubFrame& fr, long long read_ns, PyObject* err[3]);

// Phase A for a buffer the reader hub framed (HubFrame): its line items
// instead of the de-framing in pl_more; same jobs, same partial-line carry-over.
bool pl_begin_items(PipelineObject* self, const char* data, const HubFrame& fr, long long read_ns, PyObject* err[3]) {
    pl_begin(self, data, 0, read_ns, false, err);  // the per-call reset (no bytes)
    return pl_items(self, data, fr, read_ns, err);
}

// ... the items of one more hub-framed read in the same call (no reset)
bool pl_items(PipelineObject* self, const char* data, const HubFrame& fr, long long read_ns, PyObject* err[3]) {
    self->read_ns = read_ns;
    for (const HubItem& it : fr.items) {
        switch (it.kind) {
            case HI_DONE:
                self->chunk.cstate = CS_DONE;
                break;
            case HI_ERROR:
                PyErr_SetString(PyExc_ValueError, fr.error.c_str());
                PyErr_Fetch(&err[0], &err[1], &err[2]);
                return false;
            default:  // HI_LINE, HI_FRAG, HI_FRAG_END
                pl_piece(self, it.kind, data + it.off, it.len);
        }
    }
    return true;
}

// After phases B-C: counters, the newest resourceVersion, and the result
// tuple (ctrl, last_rv, logs, submits, ts), or NULL with the exception set.
PyObject* pl_end(PipelineObject* self, bool ok, PyObject* err[3]) {
    if (self->rv_span.present()) {  // before the buffer and stitched lines go away
        *self->last_rv = span_text(self->rv_span);
        self->have_rv = true;
        self->rv_known = true;
    }
    if (!ok) PyErr_Restore(err[0], err[1], err[2]);
    self->stitched->clear();
    PyObject* m = self->metrics;
    counter_add(m, "events_received", self->c_recv);
    counter_add(m, "events_filtered_critical", self->c_crit);
    counter_add(m, "events_filtered_namespace", self->c_ns);
    counter_add(m, "events_unchanged", self->c_unch);
    counter_add(m, "events_other_shard", self->c_shard);
    counter_add(m, "events_container_failure", self->c_fail);
    counter_add(m, "events_pod_condition", self->c_cond);
    counter_add(m, "events_terminating", self->c_term);
    counter_add(m, "bookmarks", self->c_bm);
    if (!ok || self->failed) {
        Py_CLEAR(self->ctrl);
        Py_CLEAR(self->logs);
        Py_CLEAR(self->submits);
        if (!PyErr_Occurred()) PyErr_SetString(PyExc_RuntimeError, "native pipeline failure");
        return nullptr;
    }
    PyObject* rv = self->have_rv ? PyUnicode_DecodeUTF8(self->last_rv->data(), (Py_ssize_t)self->last_rv->size(),
                                                       "replace")
                                 : (Py_INCREF(Py_None), Py_None);
    PyObject* logs = self->logs ? self->logs : (Py_INCREF(Py_None), Py_None);
    PyObject* subs = self->submits ? self->submits : (Py_INCREF(Py_None), Py_None);
    PyObject* ts = self->ts->empty() ? (Py_INCREF(Py_None), Py_None)
                                     : PyUnicode_FromStringAndSize(self->ts->data(), (Py_ssize_t)self->ts->size());
    PyObject* res = Py_BuildValue("(NNNNN)", self->ctrl, rv, logs, subs, ts);
    self->ctrl = self->logs = self->submits = nullptr;
    return res;
}

// Phases B-C over jobs[0, nj): workers decode ahead while this thread applies
// in order; owner[i] is the Pipeline of job i (a group batch) or NULL (all
// `self`'s). A pipeline that failed skips its remaining lines.
void pl_apply_partitioned(PipelineObject* self, LineJob* jobs, size_t nj, PipelineObject* const* owner,
                          const DecodeCfg* const* cfgs) {
    const bool probe = g_probe.on;
    const uint64_t t0 = probe ? __rdtsc() : 0;
    DecodePool* pool = self->pool;
    ParCtx ctx{jobs, owner, self, {}};
    DecodePool::Progress prog[PodStore::SHARDS];
    DecodePool::ApplyPhase ap{&par_apply_one, &ctx, PodStore::SHARDS, ctx.stop, prog};
    pool->start(jobs, (uint32_t)nj, self->cfg, cfgs, &ap);
    NotifierObject* nt = self->notifier;
    auto between = [&] {  // the loop thread services the notifier while it waits
        const NotifierCore& c = *nt->core;
        if (c.since_pump >= std::max<long long>(8, (long long)c.conns.size() * c.depth / 2)) {
            std::lock_guard<std::recursive_mutex> g(nt->core->mu);
            nt->core->pump();
        }
    };
    // The tail runs alongside the partitions: the workers walk the pod-cache
    // shards while this thread follows in stream order, counting each line
    // and submitting its notification as soon as its partition has applied
    // it — the tail (~40-80 ns per line) no longer waits for the slowest
    // partition, and the partitions no longer wait for the tail (the loop was
    // the sharded shape's bound: profiles/r5/probe). A line that needs the
    // serial path (a partition stopped at it, or a control line) waits for
    // every partition first — apply_line may touch state the walkers read
    // (a namespace seen for the first time) — and from there the rest of the
    // batch goes as before. The loop helps (walks an unclaimed partition,
    // decodes) whenever it has to wait.
    bool all_done = false;
    uint64_t t_wait = 0;
    auto wait_all = [&] {
        if (all_done) return;
        const uint64_t w0 = probe ? __rdtsc() : 0;
        pool->apply_partitions(between);
        all_done = true;
        if (probe) t_wait += __rdtsc() - w0;
    };
    // has partition p applied line i (true), or stopped at or before it (false)?
    std::unique_lock<std::recursive_mutex> nlk;
    int run = 0;
    auto applied = [&](uint8_t p, uint32_t i) {
        uint32_t v = prog[p].v.load(std::memory_order_acquire);
        if (!(v & DecodePool::DONE) && v <= i) {
            if (nlk.owns_lock()) {  // never wait holding the notifier's lock: its I/O thread needs it
                nlk.unlock();
                run = 0;
            }
            const uint64_t w0 = probe ? __rdtsc() : 0;
            uint32_t spins = 0;
            while (!((v = prog[p].v.load(std::memory_order_acquire)) & DecodePool::DONE) && v <= i) {
                if (!pool->help()) {
                    _mm_pause();
                    if ((++spins & 1023) == 0) between();
                }
            }
            if (probe) t_wait += __rdtsc() - w0;
        }
        return (v & DecodePool::DONE) ? i < (v & ~DecodePool::DONE) : true;
    };
    const uint64_t t1 = probe ? __rdtsc() : 0;
    // the serial tail — lines a partition stopped at or never took — and the
    // partitioned lines' counters, in stream order. Each job's ApplyHot was
    // last written on a worker's core: fetched TAIL_PREFETCH jobs ahead, the
    // walk no longer waits out one cross-core miss per line (~100-250 ns per
    // line of the tail: loop probe, profiles/r4)
    constexpr size_t TAIL_PREFETCH = 6;
    thread_local uint64_t epoch = 0;
    ++epoch;
    size_t npl = 0;  // distinct pipelines in the batch (a group batch has many)
    // the notifier's lock is taken once per run of up to TAIL_LOCK_RUN submits,
    // not per submit: with the notifier's I/O thread servicing sockets under
    // the same lock, a lock per notification cost the loop ~1 us each on a
    // group batch of many namespace watches (loop probe tail_submit_ns)
    // (32 beat 256 at 64 namespace watches: profiles/r4/tail_lock_run)
    constexpr int TAIL_LOCK_RUN = 32;
    if (nt) nlk = std::unique_lock<std::recursive_mutex>(nt->core->mu, std::defer_lock);
    uint64_t n_par = 0, n_serial = 0, n_sub = 0, n_runs = 0;
    PayloadTally payloads;
    for (size_t i = 0; i < nj; ++i) {
        if (i + TAIL_PREFETCH < nj) {
            __builtin_prefetch(&jobs[i + TAIL_PREFETCH].hot);
            __builtin_prefetch(reinterpret_cast<const char*>(&jobs[i + TAIL_PREFETCH].hot) + 64);
        }
        LineJob& J = jobs[i];
        PipelineObject* pl = owner ? owner[i] : self;
        if (pl->tail_epoch != epoch) {
            pl->tail_epoch = epoch;
            ++npl;
        }
        // a pipeline that failed (a serial line's apply_line raised) submits
        // nothing after that line, as the serial path; lines its partitions
        // already applied stay in the cache — the failure ends the watch and
        // the relist that follows reconciles them
        if (!pool->ready((uint32_t)i)) pool->await((uint32_t)i);
        if (pl->failed) continue;
        payloads.see(J.hot);
        const uint8_t p = J.hot.part;
        if (p != PART_SERIAL && (all_done ? i < ctx.stop[p] : applied(p, (uint32_t)i))) {
            ++n_par;
            ++pl->c_recv;
            pl->rv_fixed = false;
            const uint8_t out = J.hot.outcome;
            apply_tally(pl, out);
            if (out >= OUT_SENT) {
                const uint64_t s0 = probe ? __rdtsc() : 0;
                ++n_sub;
                const bool in_run = nt && pl->notifier == nt;  // the run's lock is this notifier's
                if (in_run && !nlk.owns_lock()) {
                    nlk.lock();
                    ++n_runs;
                }
                submit_line(pl, J, plain_names(J.hot));
                if (!in_run) {
                    pl_pump(pl, i);
                } else if (++run == TAIL_LOCK_RUN) {
                    run = 0;
                    nlk.unlock();
                    pl_pump(pl, i);
                }
                if (probe) {
                    g_probe.tail_submit += __rdtsc() - s0;
                    ++g_probe.tail_sent;
                }
            }
            continue;
        }
        pl->rv_fixed = false;
        ++n_serial;
        if (probe) ++g_probe.tail_serial;
        if (nlk.owns_lock()) {  // apply_line may call back into Python: not under the lock
            nlk.unlock();
            run = 0;
        }
        wait_all();
        apply_line(pl, J);
        pl_pump(pl, i);
    }
    if (nlk.owns_lock()) nlk.unlock();
    wait_all();  // walkers may still be scanning past their partition's last line
    pool->finish((uint32_t)nj);
    g_apply.par_batches.fetch_add(1, std::memory_order_relaxed);
    g_apply.par_lines.fetch_add(n_par, std::memory_order_relaxed);
    g_apply.tail_serial.fetch_add(n_serial, std::memory_order_relaxed);
    g_apply.tail_submits.fetch_add(n_sub, std::memory_order_relaxed);
    g_apply.tail_lock_runs.fetch_add(n_runs, std::memory_order_relaxed);
    payloads.flush();
    const uint64_t t2 = probe ? __rdtsc() : 0;
    // the resume point: the newest resourceVersion in stream order (apply_line's
    // rule), per pipeline; the walk back ends once every pipeline of the batch
    // has its own (a group batch of many namespace watches walked all of it)
    size_t fixed = 0;
    for (size_t i = nj; i-- > 0;) {
        if (i >= TAIL_PREFETCH) __builtin_prefetch(&jobs[i - TAIL_PREFETCH].hot);
        PipelineObject* pl = owner ? owner[i] : self;
        if (pl->rv_fixed) continue;
        const ApplyHot& S = jobs[i].hot;
        if (S.err || !S.obj_present || !S.rv.is_string()) continue;
        if (S.tidx == T_BOOKMARK || (S.tidx >= T_ADDED && S.tidx <= T_DELETED && S.rv.n > 2 && !pl->relist_gen)) {
            pl->rv_span = S.rv;
            pl->rv_fixed = true;
            if (!owner || ++fixed == npl) break;
        }
    }
    pl_pump(self, 0);
    if (probe) {  // apply: waiting for (and helping) the partitions; tail: this thread's own walk
        g_probe.apply += t1 - t0 + t_wait;
        const uint64_t t3 = __rdtsc();
        g_probe.tail += t3 - t1 - t_wait;
        g_probe.tail_rv += t3 - t2;
        ++g_probe.partitioned;
    }
}

void pl_decode_apply(PipelineObject* self, LineJob* jobs, size_t nj, PipelineObject* const* owner,
                     const DecodeCfg* const* cfgs) {
    const bool probe = g_probe.on;
    DecodePool* pool = self->pool;
    if (partition_ok(self, owner, nj)) {
        pl_apply_partitioned(self, jobs, nj, owner, cfgs);
        return;
    }
    g_apply.serial_batches.fetch_add(1, std::memory_order_relaxed);
    g_apply.serial_lines.fetch_add(nj, std::memory_order_relaxed);
    PayloadTally payloads;
    if (pool && nj >= PARALLEL_MIN_LINES) {
        pool->start(jobs, (uint32_t)nj, self->cfg, cfgs);
        uint64_t wait = 0, apply = 0, t = probe ? __rdtsc() : 0;
        for (size_t i = 0; i < nj; ++i) {
            PipelineObject* pl = owner ? owner[i] : self;
            if (pl->failed) {
                if (!owner) break;
                continue;
            }
            pool->await((uint32_t)i);
            const uint64_t t1 = probe ? __rdtsc() : 0;
            wait += t1 - t;
            if (i + 1 < nj && pool->ready((uint32_t)(i + 1))) {  // its apply fields, from the worker's core
                __builtin_prefetch(&jobs[i + 1].hot);
                __builtin_prefetch(reinterpret_cast<const char*>(&jobs[i + 1].hot) + 64);
            }
            payloads.see(jobs[i].hot);
            apply_line(pl, jobs[i]);
            pl_pump(pl, i);
            t = probe ? __rdtsc() : 0;
            apply += t - t1;
        }
        pool->finish((uint32_t)nj);
        if (probe) {
            g_probe.wait += wait + (__rdtsc() - t);
            g_probe.apply += apply;
        }
    } else {
        for (size_t i = 0; i < nj; ++i) {
            PipelineObject* pl = owner ? owner[i] : self;
            if (pl->failed) {
                if (!owner) break;
                continue;
            }
            decode_line(cfgs ? *cfgs[i] : *pl->cfg, jobs[i]);
            payloads.see(jobs[i].hot);
            apply_line(pl, jobs[i]);
            pl_pump(pl, i);
        }
    }
    payloads.flush();
}

// One read's bytes through phases A-C (feed / feed_chunked, and the reader
// hub's native dispatch, readerhub.inc). -> (ctrl, last_rv, logs, submits, ts)
PyObject* pl_run_impl(PipelineObject* self, const char* data, size_t len, long long read_ns, bool framed) {
    ScratchGuard scratch(self);
    const bool probe = g_probe.on;
    const uint64_t p_start = probe ? __rdtsc() : 0;
    self->njobs = 0;
    PyObject* err[3];
    const bool ok = pl_begin(self, data, len, read_ns, framed, err);
    const size_t nj = self->njobs;
    const uint64_t p_split = probe ? __rdtsc() : 0;
    if (!self->failed) pl_decode_apply(self, self->jobs_cur->data(), nj, nullptr, nullptr);
    if (probe) {
        ++g_probe.calls;
        g_probe.lines += nj;
        g_probe.bytes += (uint64_t)len;
        g_probe.split += p_split - p_start;
        if (read_ns > 0) g_probe.age_byte_ns += (long double)(mono_ns() - read_ns) * (long double)len;
    }
    PyObject* res = pl_end(self, ok, err);
    if (probe) g_probe.run += __rdtsc() - p_start;
    return res;
}

// The reader hub's grouped dispatch (readerhub.inc): reads of several bound
// streams — each Pipeline at most once — split into ONE batch of line jobs,
// decoded by the pool together and applied read by read in arrival order.
// With a thousand namespace watches a read carries ~60 lines; one decode-pool
// hand-off per read (and a notifier pump only every 256 lines *within* a
// read) made the fixed costs per line several times the cluster watch's.
struct GroupRead {
    PipelineObject* pl;
    const char* data;
    size_t len;
    long long read_ns;
    bool framed;
    const HubFrame* frame = nullptr;  // the hub framed these bytes: walk its items instead
    bool ok = true;
    PyObject* err[3] = {nullptr, nullptr, nullptr};
    size_t lo = 0, hi = 0;  // its jobs
    // Later reads of the same stream taken in the same dispatch, merged into
    // this one's call (one pl_begin / pl_end, one result): at saturation the
    // loop takes ~7 reads of the cluster watch per dispatch, and each read's
    // fixed costs — the result tuple, six counter updates in Python dicts, a
    // decode-pool hand-off — were paid per ~20 lines. Only for pipelines
    // whose submits go to the native notifier (each line keeps its own read
    // time, LineJob::read_ns).
    struct Part {
        const char* data;
        size_t len;
        long long read_ns;
        const HubFrame* frame;
    };
    std::vector<Part> more;
};

struct GroupScratch {
    std::vector<PipelineObject*> owner;
    std::vector<const DecodeCfg*> cfgs;
};
thread_local GroupScratch tl_group;

// Runs phases A-C for every read of `g`; results[k] = pl_end() of read k (NULL
// with the exception normalised into results_exc[k]). Every pipeline in `g`
// must be referenced by the caller for the duration.
void pl_run_group(std::vector<GroupRead>& g, std::vector<PyObject*>& results) {
    results.assign(g.size(), nullptr);
    if (g.empty()) return;
    const bool probe = g_probe.on;
    const uint64_t p_start = probe ? __rdtsc() : 0;
    ScratchGuard scratch(g[0].pl);  // the thread's shared jobs vector (depth 0), else g[0]'s own
    std::vector<LineJob>* jobs = g[0].pl->jobs_cur;
    size_t total = 0;
    for (GroupRead& r : g) {
        r.pl->jobs_cur = jobs;
        r.pl->njobs = total;
        r.lo = total;
        r.ok = r.frame ? pl_begin_items(r.pl, r.data, *r.frame, r.read_ns, r.err)
                       : pl_begin(r.pl, r.data, r.len, r.read_ns, r.framed, r.err);
        for (const GroupRead::Part& p : r.more) {  // a framing error ends the stream: later parts are moot
            if (!r.ok || r.pl->failed) break;
            r.ok = p.frame ? pl_items(r.pl, p.data, *p.frame, p.read_ns, r.err)
                           : pl_more(r.pl, p.data, p.len, p.read_ns, r.framed, r.err);
        }
        r.hi = r.pl->failed ? r.lo : r.pl->njobs;  // a pipeline that failed here applies nothing
        if (r.hi < r.pl->njobs) {  // drop its jobs from the batch
            r.pl->njobs = r.lo;
        }
        total = r.hi;
    }
    GroupScratch& gs = tl_group;
    gs.owner.resize(total);
    gs.cfgs.resize(total);
    for (const GroupRead& r : g)
        for (size_t i = r.lo; i < r.hi; ++i) {
            gs.owner[i] = r.pl;
            gs.cfgs[i] = r.pl->cfg;
        }
    const uint64_t p_split = probe ? __rdtsc() : 0;
    pl_decode_apply(g[0].pl, jobs->data(), total, gs.owner.data(), gs.cfgs.data());
    size_t bytes = 0;
    for (size_t k = 0; k < g.size(); ++k) {
        GroupRead& r = g[k];
        bytes += r.len;
        for (const GroupRead::Part& p : r.more) bytes += p.len;
        if (probe && r.read_ns > 0) g_probe.age_byte_ns += (long double)(mono_ns() - r.read_ns) * (long double)r.len;
        results[k] = pl_end(r.pl, r.ok, r.err);
        if (!results[k]) {  // keep each read's own exception (the next pl_end must not see it)
            PyObject *et, *ev, *tb;
            PyErr_Fetch(&et, &ev, &tb);
            PyErr_NormalizeException(&et, &ev, &tb);
            Py_XDECREF(et);
            Py_XDECREF(tb);
            results[k] = ev ? ev : PyObject_CallFunction(PyExc_RuntimeError, "s", "native pipeline failure");
            if (!results[k]) PyErr_Clear();
            r.ok = false;  // results[k] is an exception instance
        }
    }
    if (probe) {
        g_probe.calls += g.size();
        g_probe.lines += total;
        g_probe.bytes += (uint64_t)bytes;
        g_probe.split += p_split - p_start;
        g_probe.run += __rdtsc() - p_start;
    }
}

PyObject* Pipeline_feed_chunked(PipelineObject* self, PyObject* args) { return pl_run(self, args, true); }
PyObject* Pipeline_feed(PipelineObject* self, PyObject* args) { return pl_run(self, args, false); }

PyObject* Pipeline_reset(PipelineObject* self, PyObject*) {
    self->partial->clear();
    self->chunk = ChunkState();
    Py_RETURN_NONE;
}

PyObject* Pipeline_body_done(PipelineObject* self, PyObject*) { return PyBool_FromLong(self->chunk.done()); }

// last_rv() -> the newest resourceVersion the pipeline has seen (or was given), None before any
PyObject* Pipeline_last_rv(PipelineObject* self, PyObject*) {
    if (!self->rv_known) Py_RETURN_NONE;
    return PyUnicode_DecodeUTF8(self->last_rv->data(), (Py_ssize_t)self->last_rv->size(), "replace");
}

// set_last_rv(rv | None): the resume point the reflector decided (a LIST's, a checkpoint's)
PyObject* Pipeline_set_last_rv(PipelineObject* self, PyObject* arg) {
    if (arg == Py_None) {
        self->rv_known = false;
        self->last_rv->clear();
        Py_RETURN_NONE;
    }
    Py_ssize_t n;
    const char* u = PyUnicode_AsUTF8AndSize(arg, &n);
    if (!u) return nullptr;
    self->last_rv->assign(u, (size_t)n);
    self->rv_known = true;
    Py_RETURN_NONE;
}

PyObject* Pipeline_decode_threads(PipelineObject* self, PyObject*) {
    return PyLong_FromLong(self->pool ? self->pool->size() : 0);
}

PyObject* Pipeline_set_log(PipelineObject* self, PyObject* args) {
    int ev, dbg;
    if (!PyArg_ParseTuple(args, "pp", &ev, &dbg)) return nullptr;
    self->log_events = ev;
    self->log_debug = dbg;
    Py_RETURN_NONE;
}

PyObject* Pipeline_set_log_sink(PipelineObject* self, PyObject* arg) {
    if (arg != Py_None && !PyObject_TypeCheck(arg, &LogSinkType)) {
        PyErr_SetString(PyExc_TypeError, "set_log_sink: a _kwcore.LogSink or None");
        return nullptr;
    }
    Py_XINCREF(arg == Py_None ? nullptr : arg);
    Py_XSETREF(self->sink, arg == Py_None ? nullptr : (LogSinkObject*)arg);
    Py_RETURN_NONE;
}

PyObject* Pipeline_new(PyTypeObject* type, PyObject*, PyObject*) {
    PipelineObject* self = (PipelineObject*)type->tp_alloc(type, 0);
    if (!self) return nullptr;
    self->partial = new std::string();
    new (&self->chunk) ChunkState();
    self->cfg = new DecodeCfg();
    self->reasons = new ReasonSet(default_failure_reasons());
    self->cfg->reasons = self->reasons;
    self->rules = new CondRules(default_condition_rules());
    self->cfg->rules = self->rules;
    self->pool_obj = nullptr;
    self->pool = nullptr;
    self->jobs = new std::vector<LineJob>();
    self->jobs_cur = self->jobs;
    self->njobs = 0;
    self->stitched = new std::deque<std::string>();
    self->env_json = new std::string("\"\"");
    self->key = new std::string();
    self->ns_allowed = new std::vector<uint8_t>();
    self->last_rv = new std::string();
    self->ts = new std::string();
    return (PyObject*)self;
}

void Pipeline_dealloc(PipelineObject* self) {
    delete self->partial;
    self->chunk.~ChunkState();
    Py_XDECREF((PyObject*)self->pool_obj);
    delete self->cfg;
    delete self->reasons;
    delete self->rules;
    delete self->jobs;
    delete self->stitched;
    delete self->env_json;
    delete self->key;
    delete self->ns_allowed;
    delete self->ns_texts;
    delete self->last_rv;
    delete self->ts;
    Py_XDECREF((PyObject*)self->cache);
    Py_XDECREF(self->metrics);
    Py_XDECREF(self->nsset);
    Py_XDECREF((PyObject*)self->notifier);
    Py_XDECREF((PyObject*)self->sink);
    delete self->tz_utc;
    Py_XDECREF(self->repr_fallback);
    Py_TYPE(self)->tp_free((PyObject*)self);
}

int Pipeline_init(PipelineObject* self, PyObject* args, PyObject* kwds) {
    static const char* kwlist[] = {"environment", "cache", "metrics", "namespaces", "critical", "phase_mode",
                                   "shard_count", "shard_index", "shard_by_uid", "ts_utc", "notifier",
                                   "log_events", "log_debug", "decode_threads", nullptr};
    PyObject *env, *cache, *metrics, *nsset, *notifier;
    int critical, phase_mode, shard_count, shard_index, by_uid, ts_utc, log_events, log_debug;
    PyObject* decode = nullptr;  // int (private pool of that many workers) or a DecodePool
    if (!PyArg_ParseTupleAndKeywords(args, kwds, "UO!O!OppiippOpp|O", (char**)kwlist, &env, &PodCacheType, &cache,
                                     &PyDict_Type, &metrics, &nsset, &critical, &phase_mode, &shard_count,
                                     &shard_index, &by_uid, &ts_utc, &notifier, &log_events, &log_debug,
                                     &decode))
        return -1;
    DecodePoolObject* pool_obj = nullptr;
    if (decode && PyObject_TypeCheck(decode, &DecodePoolType)) {
        Py_INCREF(decode);
        pool_obj = (DecodePoolObject*)decode;
    } else if (decode && decode != Py_None) {
        long nthreads = PyLong_AsLong(decode);
        if (nthreads == -1 && PyErr_Occurred()) return -1;
        if (nthreads < 0 || nthreads > 64) {
            PyErr_SetString(PyExc_ValueError, "decode_threads must be in [0, 64] or a DecodePool");
            return -1;
        }
        if (nthreads > 0) {
            pool_obj = (DecodePoolObject*)PyObject_CallFunction((PyObject*)&DecodePoolType, "l", nthreads);
            if (!pool_obj) return -1;
        }
    }
    Py_XSETREF(self->pool_obj, pool_obj);
    self->pool = pool_obj ? pool_obj->pool : nullptr;
    PyObject* jmod = PyImport_ImportModule("json");
    PyObject* dumped = jmod ? PyObject_CallMethod(jmod, "dumps", "O", env) : nullptr;
    Py_XDECREF(jmod);
    if (!dumped) return -1;
    Py_ssize_t dn;
    const char* d = PyUnicode_AsUTF8AndSize(dumped, &dn);
    self->env_json->assign(d, (size_t)dn);
    Py_DECREF(dumped);
    Py_INCREF(cache);
    Py_XSETREF(self->cache, (PodCacheObject*)cache);
    Py_INCREF(metrics);
    Py_XSETREF(self->metrics, metrics);
    if (nsset != Py_None) {
        if (!PyAnySet_Check(nsset)) {
            PyErr_SetString(PyExc_TypeError, "namespaces must be a frozenset or None");
            return -1;
        }
        Py_INCREF(nsset);
        Py_XSETREF(self->nsset, nsset);
        // namespace filter by interned id: allowed[id] for every configured name
        // ... and for decode's payload pre-filter the same names as an
        // immutable set of texts, complete before any line is decoded
        self->ns_allowed->clear();
        NsTextSet* texts = new NsTextSet();
        self->cfg->ns_texts = texts;
        delete self->ns_texts;
        self->ns_texts = texts;
        PyObject* it = PyObject_GetIter(nsset);
        if (!it) return -1;
        PyObject* item;
        while ((item = PyIter_Next(it))) {
            std::string text;
            bool none;
            bool ok = opt_text(item, text, none);
            Py_DECREF(item);
            if (!ok) {
                Py_DECREF(it);
                return -1;
            }
            if (none) continue;
            uint32_t id = self->cache->ns->intern(text);
            if (id >= self->ns_allowed->size()) self->ns_allowed->resize(id + 1, 0);
            (*self->ns_allowed)[id] = 1;
            texts->texts.insert(std::move(text));
        }
        Py_DECREF(it);
        if (PyErr_Occurred()) return -1;
    }
    if (notifier != Py_None) {
        if (!PyObject_TypeCheck(notifier, &NotifierType)) {
            PyErr_SetString(PyExc_TypeError, "notifier must be a _kwcore.Notifier or None");
            return -1;
        }
        Py_INCREF(notifier);
        Py_XSETREF(self->notifier, (NotifierObject*)notifier);
    }
    self->critical = critical;
    self->phase_mode = phase_mode;
    self->shard_count = shard_count;
    self->shard_index = shard_index;
    self->shard_by_uid = by_uid;
    self->ts_utc = ts_utc;
    self->log_events = log_events;
    self->log_debug = log_debug;
    self->light = critical || phase_mode || self->nsset != nullptr;
    self->cfg->light = self->light || self->failures || self->conditions;
    self->cfg->critical = self->critical;
    self->cfg->env_json = self->env_json;
    self->cfg->shard_count = shard_count;
    self->cfg->shard_index = shard_index;
    self->cfg->shard_by_uid = by_uid;
    return 0;
}

// set_repr(tz_utc_repr, fallback): watcher.state_format python_repr — the
// container states rendered in C++ (pyrepr.inc) with this tzinfo repr for
// zero UTC offsets, the rest by fallback(object_bytes) -> core bytes.
PyObject* Pipeline_set_repr(PipelineObject* self, PyObject* args) {
    const char* tz;
    PyObject* fn;
    if (!PyArg_ParseTuple(args, "sO", &tz, &fn)) return nullptr;
    if (!self->tz_utc) self->tz_utc = new std::string();
    *self->tz_utc = tz;
    self->cfg->tz_utc = self->tz_utc;
    Py_INCREF(fn);
    Py_XSETREF(self->repr_fallback, fn);
    Py_RETURN_NONE;
}

// set_validate(mode): watcher.validate (0 off, 1 payload, 2 full)
PyObject* Pipeline_set_validate(PipelineObject* self, PyObject* arg) {
    long v = PyLong_AsLong(arg);
    if (PyErr_Occurred()) return nullptr;
    if (v < VALIDATE_OFF || v > VALIDATE_FULL) {
        PyErr_SetString(PyExc_ValueError, "validate mode must be 0, 1 or 2");
        return nullptr;
    }
    self->cfg->validate = (uint8_t)v;
    Py_RETURN_NONE;
}

PyObject* Pipeline_set_extra(PipelineObject* self, PyObject* arg) {
    long v = PyLong_AsLong(arg);
    if (PyErr_Occurred()) return nullptr;
    self->cfg->extra = (int)v;
    Py_RETURN_NONE;
}

// set_container_failures(on, reasons | None): watcher.alerts.container_failures
// and container_failure_reasons (None keeps the set; the extra field
// container_failures uses it too). With it on, every line is parsed
// filter-first: the findings walk the raw status spans that parse keeps.
PyObject* Pipeline_set_container_failures(PipelineObject* self, PyObject* args) {
    int on;
    PyObject* reasons = Py_None;
    if (!PyArg_ParseTuple(args, "p|O", &on, &reasons)) return nullptr;
    if (reasons != Py_None) {
        ReasonSet set;
        if (!reason_set_from(reasons, set)) return nullptr;
        *self->reasons = std::move(set);
    }
    self->failures = on;
    self->cfg->failures = on;
    self->cfg->light = self->light || on || self->conditions;
    Py_RETURN_NONE;
}

// set_pod_conditions(on, rules | None): watcher.alerts.pod_conditions and
// pod_condition_rules as (type, status, reason | None) tuples (None keeps the
// set; the extra field pod_condition_alerts uses it too). With it on, every
// line is parsed filter-first: the findings walk the raw conditions span.
PyObject* Pipeline_set_pod_conditions(PipelineObject* self, PyObject* args) {
    int on;
    PyObject* rules = Py_None;
    if (!PyArg_ParseTuple(args, "p|O", &on, &rules)) return nullptr;
    if (rules != Py_None) {
        CondRules set;
        if (!cond_rules_from(rules, set)) return nullptr;
        *self->rules = std::move(set);
    }
    self->conditions = on;
    self->cfg->conditions = on;
    self->cfg->light = self->light || on || self->failures;
    Py_RETURN_NONE;
}

PyObject* Pipeline_relist(PipelineObject* self, PyObject* args);  // relist.inc

// set_terminating(on): watcher.alerts.terminating. Nothing to walk and no
// parse to choose: parse_metadata keeps the span in both.
PyObject* Pipeline_set_terminating(PipelineObject* self, PyObject* arg) {
    const int on = PyObject_IsTrue(arg);
    if (on < 0) return nullptr;
    self->terminating = on != 0;
    self->cfg->terminating = on != 0;
    Py_RETURN_NONE;
}

// set_deadlines(on): watcher.alerts.terminating_overdue_seconds > 0. The
// decode workers compute a terminating line's deletion deadline and the apply
// stores it with the signature; off, no line does any of it.
PyObject* Pipeline_set_deadlines(PipelineObject* self, PyObject* arg) {
    const int on = PyObject_IsTrue(arg);
    if (on < 0) return nullptr;
    self->deadlines = on != 0;
    self->cfg->deadlines = on != 0;
    Py_RETURN_NONE;
}

// set_pending(on): watcher.alerts.pending_overdue_seconds > 0. The decode
// workers compute a Pending line's pending-since and build its payload core
// though nobody sends it; the apply stores the one and keeps the other.
PyObject* Pipeline_set_pending(PipelineObject* self, PyObject* arg) {
    const int on = PyObject_IsTrue(arg);
    if (on < 0) return nullptr;
    self->pending = on != 0;
    self->cfg->pending = on != 0;
    Py_RETURN_NONE;
}

// set_unready(on): watcher.alerts.unready_overdue_seconds > 0. The decode
// workers compute a Running line's unready-since and build its payload core
// though nobody sends it; the apply stores the one and keeps the other.
PyObject* Pipeline_set_unready(PipelineObject* self, PyObject* arg) {
    const int on = PyObject_IsTrue(arg);
    if (on < 0) return nullptr;
    self->unready = on != 0;
    self->cfg->unready = on != 0;
    Py_RETURN_NONE;
}

PyObject* Pipeline_report_overdue(PipelineObject* self, PyObject* args, PyObject* kwargs);  // relist.inc

PyMethodDef Pipeline_methods[] = {
    {"relist", (PyCFunction)Pipeline_relist, METH_VARARGS,
     "relist(scope_ns, notify) -> Relist: reconcile a LIST of the scope against the cache (relist.inc)"},
    {"set_extra", (PyCFunction)Pipeline_set_extra, METH_O, "set_extra(mask): watcher.payload_extra_fields"},
    {"set_validate", (PyCFunction)Pipeline_set_validate, METH_O, "set_validate(0 off | 1 payload | 2 full)"},
    {"set_container_failures", (PyCFunction)Pipeline_set_container_failures, METH_VARARGS,
     "set_container_failures(on, reasons=None): watcher.alerts.container_failures / container_failure_reasons"},
    {"set_pod_conditions", (PyCFunction)Pipeline_set_pod_conditions, METH_VARARGS,
     "set_pod_conditions(on, rules=None): watcher.alerts.pod_conditions / pod_condition_rules"},
    {"set_terminating", (PyCFunction)Pipeline_set_terminating, METH_O, "set_terminating(on): watcher.alerts.terminating"},
    {"set_deadlines", (PyCFunction)Pipeline_set_deadlines, METH_O,
     "set_deadlines(on): watcher.alerts.terminating_overdue_seconds > 0"},
    {"set_pending", (PyCFunction)Pipeline_set_pending, METH_O,
     "set_pending(on): watcher.alerts.pending_overdue_seconds > 0"},
    {"set_unready", (PyCFunction)Pipeline_set_unready, METH_O,
     "set_unready(on): watcher.alerts.unready_overdue_seconds > 0"},
    {"report_overdue", (PyCFunction)(void (*)(void))Pipeline_report_overdue, METH_VARARGS | METH_KEYWORDS,
     "report_overdue(now_s, after_s, scope_ns, read_ns, pending=False) -> (sent, ctrl, logs, submits): the overdue "
     "sweep, of the terminating pods or of the Pending ones (relist.inc)"},
    {"set_repr", (PyCFunction)Pipeline_set_repr, METH_VARARGS,
     "set_repr(tz_utc_repr, fallback): state_format python_repr (pyrepr.inc)"},
    {"feed_chunked", (PyCFunction)Pipeline_feed_chunked, METH_VARARGS,
     "feed_chunked(data, read_ns) -> (ctrl, last_rv, logs, submits, ts)"},
    {"feed", (PyCFunction)Pipeline_feed, METH_VARARGS, "feed(data, read_ns): unframed NDJSON"},
    {"reset", (PyCFunction)Pipeline_reset, METH_NOARGS, "drop partial line / chunk state"},
    {"body_done", (PyCFunction)Pipeline_body_done, METH_NOARGS, "terminating chunk seen"},
    {"last_rv", (PyCFunction)Pipeline_last_rv, METH_NOARGS, "newest resourceVersion seen, or None"},
    {"set_last_rv", (PyCFunction)Pipeline_set_last_rv, METH_O, "set_last_rv(rv | None)"},
    {"set_log", (PyCFunction)Pipeline_set_log, METH_VARARGS, "set_log(log_events, log_debug)"},
    {"set_log_sink", (PyCFunction)Pipeline_set_log_sink, METH_O, "set_log_sink(LogSink | None): lines written natively"},
    {"decode_threads", (PyCFunction)Pipeline_decode_threads, METH_NOARGS, "worker threads in the decode pool"},
    {nullptr, nullptr, 0, nullptr}};

PyTypeObject PipelineType = {PyVarObject_HEAD_INIT(nullptr, 0)};

// _kwcore.probe(enable) -> totals since the previous call (ns), then resets.
// _kwcore.set_partitioned_apply(on) -> previous setting (watcher.partitioned_apply)
PyObject* kw_set_partitioned_apply(PyObject*, PyObject* arg) {
    const int on = PyObject_IsTrue(arg);
    if (on < 0) return nullptr;
    const bool prev = g_partitioned_apply;
    g_partitioned_apply = on;
    return PyBool_FromLong(prev);
}

// _kwcore.set_payload_prefilter(on) -> previous setting. Default on; off
// builds every payload the critical filter keeps, as before the pre-filter:
// for the tests that pin the two to one output and for A/B runs. Not to be
// flipped while a batch is being decoded.
PyObject* kw_set_payload_prefilter(PyObject*, PyObject* arg) {
    const int on = PyObject_IsTrue(arg);
    if (on < 0) return nullptr;
    const bool prev = g_payload_prefilter;
    g_payload_prefilter = on;
    return PyBool_FromLong(prev);
}

// _kwcore.apply_partition(uid) -> the partition (pod-cache shard) that applies
// a pod's lines in a partitioned batch; for tests that must fill every one
PyObject* kw_apply_partition(PyObject*, PyObject* arg) {
    Py_ssize_t n;
    const char* u = PyUnicode_Check(arg) ? PyUnicode_AsUTF8AndSize(arg, &n) : nullptr;
    if (!u) {
        if (!PyErr_Occurred()) PyErr_SetString(PyExc_TypeError, "uid must be a str");
        return nullptr;
    }
    return PyLong_FromLong((long)PodStore::shard_of(sv_hash(std::string_view(u, (size_t)n))));
}

// _kwcore.apply_stats() -> cumulative counts of the apply paths (ApplyStats)
PyObject* kw_apply_stats(PyObject*, PyObject*) {
    auto v = [](const std::atomic<uint64_t>& a) { return (unsigned long long)a.load(std::memory_order_relaxed); };
    return Py_BuildValue("{s:K,s:K,s:K,s:K,s:K,s:K,s:K,s:K,s:K}", "partitioned_batches", v(g_apply.par_batches),
                         "partitioned_lines", v(g_apply.par_lines), "tail_serial_lines", v(g_apply.tail_serial),
                         "tail_submits", v(g_apply.tail_submits), "tail_lock_runs", v(g_apply.tail_lock_runs),
                         "serial_batches", v(g_apply.serial_batches), "serial_lines", v(g_apply.serial_lines),
                         "payload_built", v(g_apply.payload_built), "payload_prefiltered",
                         v(g_apply.payload_prefiltered));
}

PyObject* kw_probe(PyObject*, PyObject* arg) {
    const int on = PyObject_IsTrue(arg);
    if (on < 0) return nullptr;
    Probe& P = g_probe;
    const int64_t now = mono_ns();
    const uint64_t tsc = __rdtsc();
    PyObject* out;
    if (P.t0_ns && now > P.t0_ns) {
        const double per_ns = (double)(tsc - P.t0_tsc) / (double)(now - P.t0_ns);  // TSC ticks per ns
        auto ns = [per_ns](uint64_t ticks) { return (long long)((double)ticks / per_ns); };
        out = Py_BuildValue("{s:L,s:K,s:K,s:K,s:L,s:L,s:L,s:L,s:K,s:L,s:d,s:L,s:L,s:K}", "wall_ns", (long long)(now - P.t0_ns),
                            "calls", (unsigned long long)P.calls, "lines", (unsigned long long)P.lines, "bytes",
                            (unsigned long long)P.bytes, "split_ns", ns(P.split), "wait_ns", ns(P.wait), "apply_ns",
                            ns(P.apply), "run_ns", ns(P.run), "notifier_io_calls", (unsigned long long)P.nio_calls,
                            "notifier_io_ns", ns(P.nio), "data_age_us",
                            P.bytes ? (double)(P.age_byte_ns / (long double)P.bytes) / 1e3 : 0.0,
                            "pump_ns", ns(P.pump), "tail_ns", ns(P.tail), "partitioned_batches",
                            (unsigned long long)P.partitioned);
        if (out) {
            PyObject* extra = Py_BuildValue("{s:K,s:K,s:L,s:L}", "tail_serial_lines", (unsigned long long)P.tail_serial,
                                            "tail_sent", (unsigned long long)P.tail_sent, "tail_submit_ns",
                                            ns(P.tail_submit), "tail_rv_ns", ns(P.tail_rv));
            if (!extra || PyDict_Update(out, extra) < 0) {
                Py_XDECREF(extra);
                Py_DECREF(out);
                return nullptr;
            }
            Py_DECREF(extra);
        }
    } else {
        out = PyDict_New();
    }
    P = Probe();
    P.on = on;
    P.t0_ns = now;
    P.t0_tsc = tsc;
    return out;
}

int register_pipeline(PyObject* m) {
    DecodePoolType.tp_name = "_kwcore.DecodePool";
    DecodePoolType.tp_basicsize = sizeof(DecodePoolObject);
    DecodePoolType.tp_flags = Py_TPFLAGS_DEFAULT;
    DecodePoolType.tp_doc = "DecodePool(threads): worker threads for Pipeline decode (phase B)";
    DecodePoolType.tp_methods = DecodePool_methods;
    DecodePoolType.tp_new = DecodePool_new;
    DecodePoolType.tp_init = (initproc)DecodePool_init;
    DecodePoolType.tp_dealloc = (destructor)DecodePool_dealloc;
    if (PyType_Ready(&DecodePoolType) < 0) return -1;
    Py_INCREF(&DecodePoolType);
    PyModule_AddObject(m, "DecodePool", (PyObject*)&DecodePoolType);
    PipelineType.tp_name = "_kwcore.Pipeline";
    PipelineType.tp_basicsize = sizeof(PipelineObject);
    PipelineType.tp_flags = Py_TPFLAGS_DEFAULT;
    PipelineType.tp_doc = "Native fused decode + event pipeline (see engine/pipeline.py)";
    PipelineType.tp_methods = Pipeline_methods;
    PipelineType.tp_new = Pipeline_new;
    PipelineType.tp_init = (initproc)Pipeline_init;
    PipelineType.tp_dealloc = (destructor)Pipeline_dealloc;
    if (PyType_Ready(&PipelineType) < 0) return -1;
    Py_INCREF(&PipelineType);
    PyModule_AddObject(m, "Pipeline", (PyObject*)&PipelineType);
    return 0;
}
