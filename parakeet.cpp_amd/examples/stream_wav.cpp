// examples/stream_wav.cpp -- the reference's streaming usage (README "Streaming": NemotronTranscriber t(weights, vocab, cfg);
// t.to_gpu(); while (...) text += t.transcribe_chunk(pcm, n);) on the MI355X engine.
// usage: stream_wav <model.safetensors> <vocab.txt> <audio.wav> <layers> [chunk_samples=2560] [latency_frames=1]
//        [--spot "phrase"]... [--spot-min-score x] [--spot-patience frames] [--endpoint [--endpoint-min-silence-ms n] [--eou-token id]]
// --endpoint watches for the end of every utterance while the audio is transcribed; one line per finished utterance is printed on stderr.
// --spot (repeatable) watches the audio for the phrase while it is transcribed; every hit is printed on stderr as it leaves.
// (<layers>: number of encoder layers of the weights file -- tests use a 2-layer cut of the nemotron-600m architecture).
// Prints one JSON object: the chunk texts joined, get_text(), and the token ids with their absolute frames.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <vector>

#include <parakeet/parakeet.hpp>

int main(int argc, char **argv) {
    std::vector<std::string> phrases;
    parakeet::StreamSpotOptions spot;
    parakeet::EndpointOptions ep;
    bool endpoint = false;
    {   // the options leave argv; the positional arguments keep their places
        int k = 1;
        for (int i = 1; i < argc; ++i) {
            if (!std::strcmp(argv[i], "--spot") && i + 1 < argc) phrases.push_back(argv[++i]);
            else if (!std::strcmp(argv[i], "--spot-min-score") && i + 1 < argc) spot.min_score = (float)std::atof(argv[++i]);
            else if (!std::strcmp(argv[i], "--spot-patience") && i + 1 < argc) spot.patience = std::atoi(argv[++i]);
            else if (!std::strcmp(argv[i], "--endpoint")) endpoint = true;
            else if (!std::strcmp(argv[i], "--endpoint-min-silence-ms") && i + 1 < argc) ep.min_silence_ms = std::atoi(argv[++i]);
            else if (!std::strcmp(argv[i], "--eou-token") && i + 1 < argc) ep.eou_token_id = std::atoi(argv[++i]);
            else argv[k++] = argv[i];
        }
        argc = k;
    }
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s model.safetensors vocab.txt audio.wav layers [chunk_samples] [latency_frames]\n", argv[0]);
        return 2;
    }
    try {
        const int chunk = argc > 5 ? std::atoi(argv[5]) : 2560, latency = argc > 6 ? std::atoi(argv[6]) : 1;
        auto cfg = parakeet::make_nemotron_600m_config(latency);
        cfg.encoder.num_layers = std::atoi(argv[4]);
        parakeet::NemotronTranscriber t(argv[1], argv[2], cfg);
        t.to_gpu();
        float *pcm = nullptr;
        int64_t n = 0;
        int sr = 0;
        parakeet::detail::check(pk_read_wav(argv[3], &pcm, &n, &sr));
        std::string joined;
        if (!phrases.empty()) t.set_keywords(phrases, spot);
        std::vector<parakeet::SpotEvent> hits;
        size_t shown = 0;
        auto show = [&] {
            for (; shown < hits.size(); ++shown)
                std::fprintf(stderr, "spot: \"%s\" %.2f s .. %.2f s  score %.4f\n", phrases[hits[shown].keyword].c_str(), hits[shown].start, hits[shown].end,
                             hits[shown].score);
        };
        if (endpoint && !phrases.empty()) {
            std::fprintf(stderr, "--endpoint and --spot: one of the two (the C call pk_stream_push_endpoint serves both at once)\n");
            pk_free(pcm);
            return 2;
        }
        if (endpoint) t.set_endpointing(ep);
        std::vector<parakeet::Utterance> utts;
        size_t told = 0;
        static const char *const why[] = {"", "silence", "max length", "token"};
        for (int64_t off = 0; off + chunk <= n; off += chunk) {
            if (endpoint) {
                joined += t.transcribe_chunk_endpoint(pcm + off, (size_t)chunk, utts);
                for (; told < utts.size(); ++told)
                    std::fprintf(stderr, "utterance: %.2f s .. %.2f s (%s, %zu tokens) \"%s\"\n", utts[told].start, utts[told].end,
                                 why[utts[told].reason & 3], utts[told].ids.size(), utts[told].text.c_str());
            } else if (phrases.empty()) joined += t.transcribe_chunk(pcm + off, (size_t)chunk);
            else { joined += t.transcribe_chunk_spot(pcm + off, (size_t)chunk, hits); show(); }
        }
        if (!phrases.empty()) { t.flush_spots(hits); show(); }
        pk_free(pcm);
        auto esc = [](const std::string &s) { std::string o; for (char c : s) { if (c == '"' || c == '\\') o += '\\'; o += c; } return o; };
        std::printf("{\"joined\": \"%s\", \"text\": \"%s\", \"tokens\": [", esc(joined).c_str(), esc(t.get_text()).c_str());
        const auto &tt = t.get_timestamped_tokens();
        for (size_t i = 0; i < tt.size(); ++i) std::printf("%s[%d, %d, %d]", i ? ", " : "", tt[i].token_id, tt[i].start_frame, tt[i].end_frame);
        std::printf("]}\n");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
