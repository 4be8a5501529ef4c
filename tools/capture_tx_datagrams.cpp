// Test infrastructure only (tools/capture_tx_datagrams.py builds and runs it on the CPU; nothing built from
// it is committed): the two-endpoint loopback of tools/capture_datagrams.cpp on the reference's unchanged
// protocol layer and the reference codec, recording the server's side of the traffic for
// tests/golden/tx_datagrams.npz:
//   record type 0   every datagram the server's SendData was given, before the driver's deterministic 10 %
//                   loss, pong prefix and all, in send order
//   record type 1   every payload handed to the server's Send, in order
//   record type 2   every message handed to the server's SendOOB
// The loss and the client stay in, so that the server's loss estimate and its amount of recovery behave as
// in that capture.
// Each record is [type u8][len u16 LE][bytes] in the file named by --out. The server sends --per-tick
// payloads of 8..--max-bytes bytes every 5 ms ([u32 id][PCG32 stream]) and an out-of-band message every 40
// ticks; the run lasts --seconds (more than the reference's 1 s statistics interval, so that pong prefixes
// occur), then drains.
#include "Shorthair.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

using namespace cat::shorthair;

namespace {

struct Pcg32 {  // PCG-XSH-RR
    uint64_t state = 0, inc = 0;
    void seed(uint64_t y, uint64_t x = 0) {
        state = 0;
        inc = (y << 1u) | 1u;
        next();
        state += x;
        next();
    }
    uint32_t next() {
        const uint64_t old = state;
        state = old * 6364136223846793005ULL + inc;
        const uint32_t xs = static_cast<uint32_t>(((old >> 18) ^ old) >> 27);
        const uint32_t rot = static_cast<uint32_t>(old >> 59);
        return (xs >> rot) | (xs << ((0u - rot) & 31u));
    }
};

std::FILE *g_out = nullptr;

void record(int type, const uint8_t *data, int bytes) {
    const uint8_t head[3] = {static_cast<uint8_t>(type), static_cast<uint8_t>(bytes & 255),
                             static_cast<uint8_t>(bytes >> 8)};
    std::fwrite(head, 1, 3, g_out);
    std::fwrite(data, 1, static_cast<size_t>(bytes), g_out);
}

struct Endpoint : IShorthair {
    ShorthairCodec codec;
    Endpoint *peer = nullptr;
    bool is_server = false;
    uint64_t lcg = 0x9E3779B97F4A7C15ULL;
    long wire_sent = 0, wire_dropped = 0, delivered = 0, oob = 0;
    std::vector<uint8_t> scratch = std::vector<uint8_t>(4096);

    void OnPacket(uint8_t *, int) override {
        if (!is_server) ++delivered;
    }
    void OnOOB(uint8_t *, int) override {
        if (!is_server) ++oob;
    }
    void SendData(uint8_t *buffer, int bytes) override {
        ++wire_sent;
        if (is_server) {
            record(0, buffer, bytes);
            lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL;
            if ((lcg >> 33) % 10 == 0) {  // 10 % loss
                ++wire_dropped;
                return;
            }
        }
        std::memcpy(scratch.data(), buffer, static_cast<size_t>(bytes));  // Recv modifies its buffer
        peer->codec.Recv(scratch.data(), bytes);
    }
};

}  // namespace

int main(int argc, char **argv) {
    double seconds = 1.3;
    int per_tick = 4, max_bytes = 40;
    const char *out = nullptr;
    for (int i = 1; i + 1 < argc; i += 2) {
        if (std::strcmp(argv[i], "--seconds") == 0) seconds = std::atof(argv[i + 1]);
        if (std::strcmp(argv[i], "--per-tick") == 0) per_tick = std::atoi(argv[i + 1]);
        if (std::strcmp(argv[i], "--max-bytes") == 0) max_bytes = std::atoi(argv[i + 1]);
        if (std::strcmp(argv[i], "--out") == 0) out = argv[i + 1];
    }
    if (!out || !(g_out = std::fopen(out, "wb")) || max_bytes < 8 || max_bytes > 1350) {
        std::fprintf(stderr, "usage: capture_tx_datagrams --out FILE [--seconds S] [--per-tick N] [--max-bytes B]\n");
        return 2;
    }
    Endpoint server, client;
    server.peer = &client;
    client.peer = &server;
    server.is_server = true;
    Settings ss, cs;
    ss.min_fec_overhead = cs.min_fec_overhead = 0.2f;
    ss.max_delay = cs.max_delay = 100;
    ss.max_data_size = 1350;
    cs.max_data_size = 1400;
    ss.interface_ptr = &server;
    cs.interface_ptr = &client;
    if (!server.codec.Initialize(ss) || !client.codec.Initialize(cs)) {
        std::printf("{\"error\": \"Initialize failed\"}\n");
        return 2;
    }
    Pcg32 lens;
    lens.seed(4321);
    uint32_t next_id = 0;
    std::vector<uint8_t> buf(1400);
    const auto t0 = std::chrono::steady_clock::now();
    for (int tick = 0; std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < seconds; ++tick) {
        std::this_thread::sleep_for(std::chrono::milliseconds(5));
        client.codec.Tick();
        server.codec.Tick();
        if (tick % 40 == 7) {
            const uint8_t msg[6] = {0x05, 'o', 'o', 'b', static_cast<uint8_t>(tick & 255), static_cast<uint8_t>(tick >> 8)};
            record(2, msg, sizeof(msg));
            server.codec.SendOOB(msg, sizeof(msg));
        }
        for (int i = 0; i < per_tick; ++i) {
            const int len = 8 + static_cast<int>(lens.next() % static_cast<uint32_t>(max_bytes - 8 + 1));
            const uint32_t id = next_id++;
            std::memcpy(buf.data(), &id, 4);
            for (int j = 4; j < len; ++j) buf[static_cast<size_t>(j)] = static_cast<uint8_t>(lens.next());
            record(1, buf.data(), len);
            server.codec.Send(buf.data(), static_cast<size_t>(len));
        }
    }
    for (int i = 0; i < 60; ++i) {  // drain: the last group's recovery packets go out and are decoded
        std::this_thread::sleep_for(std::chrono::milliseconds(5));
        client.codec.Tick();
        server.codec.Tick();
    }
    std::printf("{\"sent\": %u, \"delivered\": %ld, \"oob_delivered\": %ld, \"wire_packets\": %ld, \"wire_dropped\": %ld}\n",
                next_id, client.delivered, client.oob, server.wire_sent, server.wire_dropped);
    server.codec.Finalize();
    client.codec.Finalize();
    std::fclose(g_out);
    return 0;
}
