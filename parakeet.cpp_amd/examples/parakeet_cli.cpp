// examples/parakeet_cli.cpp -- the reference's command line (src/main.cpp:12-37, :642-727) on the MI355X engine: same positional
// arguments, --model types and options; every model type runs through the drop-in facade classes.
//   parakeet_cli <model.safetensors> <audio.wav> [--model TYPE] [--ctc|--tdt] [--vocab PATH] [--timestamps] [--boost PHRASE]...
//                [--boost-score N] [--sortformer-weights PATH] [--latency N] [--streaming] [--gpu] [--beam W [--nbest N] [--prune K] [--beam-head ctc|tdt]]
//                [--align "text" | --align-file path.txt] [--align-head ctc|tdt] [--score "text"] [--nbest N --rescore-tdt W]
//                [--spot "phrase"]... [--spot-file path.txt] [--spot-head ctc|tdt] [--spot-hits N] [--spot-min-score X] [--lm file.arpa [--lm-alpha A] [--lm-beta B]]
//                [--device-resample] [--vad [--vad-max-piece S]]
//                [--nlm file.safetensors --nlm-heads H --nlm-bos ID [--nlm-eos ID] [--nlm-alpha A] [--nlm-beta B]]
// New: --vad (tdt-ctc-110m, tdt-600m; 16 kHz) cuts the file at its pauses on the device and transcribes only the speech, in pieces of at most
// S seconds (--vad-max-piece S, default 30) that share batches (TranscribeOptions::vad): for long or sparse recordings.
// New: --device-resample (tdt-ctc-110m, tdt-600m) reads the file at its own sample rate and resamples it to 16 kHz on the device, inside the call
// (Transcriber::set_device_resampling), instead of on the host while the file is read.
// New: --beam W (with --ctc / --decoder ctc, tdt-ctc-110m) runs the CTC prefix beam search and prints the N best hypotheses with scores.
// New: --align "text" / --align-file path.txt (tdt-ctc-110m, tdt-600m) aligns the given transcript with the audio (CTC forced alignment) and
// prints its word timestamps in the format of --timestamps.  --align-head tdt aligns through the TDT head instead (the default stays ctc): the one
// that works for tdt-600m, which has no CTC head.
// New: --score "text" (tdt-ctc-110m, tdt-600m) prints the log-likelihood of the given transcript under the TDT head (the forward algorithm on the
// alignment's lattice).  --nbest N --rescore-tdt W (tdt-ctc-110m) prints the N best hypotheses of the CTC beam search re-ranked by
// (1 - W) * CTC score + W * TDT log-likelihood, with both parts.
// New: --spot "phrase" (repeatable) / --spot-file path.txt (one phrase per line) (tdt-ctc-110m) searches the audio for every phrase (CTC keyword
// spotting) and prints one line per hit: phrase<TAB>start<TAB>end<TAB>score (seconds; score <= 0, 0 = the greedy path over the span is the phrase).
// --spot-hits N: up to N non-overlapping hits per phrase (default 1); --spot-min-score X: only hits with score >= X (default: no threshold).
// New: --spot-head tdt (tdt-ctc-110m, tdt-600m) spots through the TDT head, which needs no CTC head; a phrase is scored as if it began the utterance.
// New: --lm file.arpa (with --beam W and the CTC decoder, or with --beam W --beam-head tdt) fuses an n-gram language model over token ids into the beam search (shallow fusion):
// hypotheses rank by acoustic score + LM score, LM score = sum per token of A * log p + B (--lm-alpha A, default 0.5; --lm-beta B, default 0);
// both parts are printed.  tools/make_token_corpus.py turns text into the id lines an n-gram trainer makes such a file from.
// New: --nlm file.safetensors --nlm-heads H --nlm-bos ID [--nlm-eos ID] (with --beam W and the CTC decoder, or with --beam W --beam-head tdt) re-ranks the
// N best hypotheses with a causal Transformer LM over token ids: combined = acoustic + A * LM + B * tokens (--nlm-alpha A,
// default 0.5; --nlm-beta B, default 0); the rest of the LM's configuration is read off the file's tensor shapes; all three values are printed.
// Differences: --gpu is accepted and implied (there is no CPU path); --features (a .npy of pre-computed features) is not supported.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <string>
#include <vector>

#include <parakeet/parakeet.hpp>

using namespace parakeet;
using Clock = std::chrono::high_resolution_clock;

static void usage(const char *prog) {
    std::cerr << "Usage: " << prog << " <model.safetensors> <audio.wav> [options]\n"
              << "  --model TYPE   tdt-ctc-110m (default), tdt-600m, rnnt-600m, eou-120m, nemotron-600m, sortformer, diarized\n"
              << "  --ctc | --tdt | --decoder ctc|tdt  decoder (default: TDT)\n"
              << "  --beam W [--nbest N] [--prune K]  CTC prefix beam search (needs the CTC decoder), N best hypotheses\n"
              << "  --align \"text\" | --align-file path.txt  CTC forced alignment of a known transcript: its word timestamps\n"
              << "  --beam W --beam-head tdt [--nbest N]  TDT beam search (tdt-ctc-110m, tdt-600m), N best hypotheses with path scores\n"
              << "  --align-head ctc|tdt  the head --align goes through (default: ctc; tdt needs no CTC head)\n"
              << "  --score \"text\"  log-likelihood of a known transcript under the TDT head\n"
              << "  --nbest N --rescore-tdt W  the N best hypotheses re-ranked by (1 - W) * CTC score + W * TDT log-likelihood\n"
              << "  --spot \"phrase\" (repeatable) | --spot-file path.txt  where was each phrase said: phrase<TAB>start<TAB>end<TAB>score per hit\n"
              << "  --beam W --lm file.arpa [--lm-alpha A] [--lm-beta B]  the CTC beam search fused with an n-gram model over token ids\n"
              << "  --beam W --beam-head tdt --lm file.arpa [--lm-alpha A] [--lm-beta B]  the TDT beam search fused with the model; both scores per hypothesis\n"
              << "  --beam W [--beam-head tdt] --nbest N --nlm file.safetensors --nlm-heads H --nlm-bos ID [--nlm-eos ID] [--nlm-alpha A] [--nlm-beta B]\n"
              << "                      the N best hypotheses re-ranked by a Transformer LM over token ids: am + A * nlm + B * tokens\n"
              << "  --spot-hits N (default 1), --spot-min-score X (<= 0; default: no threshold), --spot-head ctc|tdt (default ctc; tdt works for tdt-600m)\n"
              << "  --device-resample  resample files that are not 16 kHz on the device instead of on the host (tdt-ctc-110m, tdt-600m)\n"
              << "  --vad [--vad-max-piece S]  transcribe only the speech, cut at the pauses into pieces of at most S seconds (default 30)\n"
              << "  --boost PHRASE (repeatable), --boost-score N (default 5.0)\n"
              << "  --vocab PATH, --sortformer-weights PATH, --timestamps, --streaming, --latency N (0/1/6/13), --gpu\n";
}

static void print_result(const TranscribeResult &r, bool timestamps, double ms) {
    std::cout << "Inference: " << std::fixed << std::setprecision(1) << ms << " ms\n";
    std::cout << "\n--- Transcription ---\n" << r.text << "\n";
    std::cout << "Tokens (" << r.token_ids.size() << "):";
    for (int id : r.token_ids) std::cout << ' ' << id;
    std::cout << "\n";
    if (timestamps) {
        std::cout << "\n--- Word timestamps ---\n";
        for (const auto &w : r.word_timestamps)
            std::cout << "  [" << std::fixed << std::setprecision(2) << w.start << "s - " << w.end << "s] (" << std::setprecision(3) << w.confidence << ") " << w.word << "\n";
    }
}

// --align: the given transcript's word timestamps, in the format of --timestamps
template <class T>
static int run_align(T &t, const std::string &audio_path, const std::string &text, bool tdt_head) {
    const auto t0 = Clock::now();
    const auto r = tdt_head ? t.align_tdt(audio_path, text) : t.align(audio_path, text);
    const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
    if (!r.aligned) {
        std::cerr << "Error: the transcript (" << r.token_ids.size() << " tokens) cannot be aligned with this audio\n";
        return 1;
    }
    if (tdt_head) std::cout << "Alignment (tdt): score " << std::setprecision(9) << std::defaultfloat << r.score << "\n";
    else std::cout << "Alignment: score " << std::setprecision(9) << std::defaultfloat << r.score << " log-likelihood " << r.total << "\n";
    print_result(r, true, ms);
    return 0;
}

// --score: the transcript's log-likelihood under the TDT head
template <class T>
static int run_score(T &t, const std::string &audio_path, const std::string &text) {
    const auto r = t.score(audio_path, text, /*tdt_head=*/true);
    if (!r.scored) {
        std::cerr << "Error: no path of the TDT head emits the transcript (" << r.token_ids.size() << " tokens) on this audio\n";
        return 1;
    }
    std::cout << "Score (tdt): log-likelihood " << std::fixed << std::setprecision(4) << r.log_likelihood << "\n";
    std::cout << "Tokens (" << r.token_ids.size() << "):";
    for (int id : r.token_ids) std::cout << ' ' << id;
    std::cout << "\n";
    return 0;
}

// --spot: one line per hit, phrase<TAB>start<TAB>end<TAB>score, phrases in the order given, a phrase's hits best first
template <class T>
static int run_spot(T &t, const std::string &audio_path, const std::vector<std::string> &phrases, const SpotOptions &so, bool tdt) {
    const auto hits = tdt ? t.spot_tdt(audio_path, phrases, so) : t.spot(audio_path, phrases, so);
    std::cout << "Spotting" << (tdt ? " (tdt): " : ": ") << phrases.size() << " phrases\n";
    for (size_t k = 0; k < phrases.size(); ++k)
        for (const auto &h : hits[k])
            std::cout << phrases[k] << '\t' << std::setprecision(9) << std::defaultfloat << h.start << '\t' << h.end << '\t' << h.score << "\n";
    return 0;
}

template <class T>
static int run_stream(T &t, const std::string &audio_path, bool timestamps) {
    t.to_gpu();
    const auto audio = read_audio(audio_path);
    const size_t chunk = 2560;                                      // 160 ms at 16 kHz (main.cpp run_*_streaming)
    const auto t0 = Clock::now();
    for (size_t off = 0; off < audio.samples.size(); off += chunk) {
        const size_t n = std::min(chunk, audio.samples.size() - off);
        const std::string piece = t.transcribe_chunk(audio.samples.data() + off, n);
        if (!piece.empty()) std::cout << piece << std::flush;
    }
    const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
    std::cout << "\nStreaming: " << std::fixed << std::setprecision(1) << ms << " ms for " << audio.duration << " s\n";
    std::cout << "\n--- Transcription ---\n" << t.get_text() << "\n";
    if (timestamps)
        for (const auto &tk : t.get_timestamped_tokens())
            std::cout << "  token " << tk.token_id << " frames [" << tk.start_frame << ", " << tk.end_frame << "]\n";
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 3) { usage(argv[0]); return 1; }
    try {
        const std::string weights = argv[1], audio_path = argv[2];
        std::string model = "tdt-ctc-110m", vocab, sf_weights, align_text, score_text, lm_path, nlm_path;
        LmOptions lm_opts;
        NlmOptions nlm_opts;
        int nlm_heads = 0, nlm_bos = -1, nlm_eos = -1;
        bool use_ctc = false, timestamps = false, device_resample = false, align = false, align_tdt = false, beam_tdt = false, score = false, rescore = false, nbest_given = false;
        int latency = 0, beam = 0, nbest = 1, prune = 16;
        float rescore_w = 0.5f;
        std::vector<std::string> boost, spot;
        SpotOptions spot_opts;
        float boost_score = 5.0f, vad_max_piece = 30.0f;
        bool vad = false, spot_tdt = false;
        for (int i = 3; i < argc; ++i) {
            const std::string a = argv[i];
            if (a == "--model" && i + 1 < argc) model = argv[++i];
            else if (a == "--ctc") use_ctc = true;
            else if (a == "--tdt") use_ctc = false;
            else if (a == "--decoder" && i + 1 < argc) {
                const std::string d = argv[++i];
                if (d != "ctc" && d != "tdt") { std::cerr << "Unknown decoder: " << d << "\n"; return 1; }
                use_ctc = d == "ctc";
            }
            else if (a == "--beam" && i + 1 < argc) beam = std::stoi(argv[++i]);
            else if (a == "--align" && i + 1 < argc) { align_text = argv[++i]; align = true; }
            else if (a == "--align-file" && i + 1 < argc) {
                std::ifstream f(argv[++i]);
                if (!f) { std::cerr << "Error: cannot open " << argv[i] << "\n"; return 1; }
                align_text.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
                while (!align_text.empty() && (align_text.back() == '\n' || align_text.back() == '\r')) align_text.pop_back();
                align = true;
            }
            else if (a == "--align-head" && i + 1 < argc) {
                const std::string hd = argv[++i];
                if (hd != "ctc" && hd != "tdt") { std::cerr << "Unknown alignment head: " << hd << "\n"; return 1; }
                align_tdt = hd == "tdt";
            }
            else if (a == "--beam-head" && i + 1 < argc) {
                const std::string hd = argv[++i];
                if (hd != "ctc" && hd != "tdt") { std::cerr << "Unknown beam head: " << hd << "\n"; return 1; }
                beam_tdt = hd == "tdt";
            }
            else if (a == "--nbest" && i + 1 < argc) { nbest = std::stoi(argv[++i]); nbest_given = true; }
            else if (a == "--score" && i + 1 < argc) { score_text = argv[++i]; score = true; }
            else if (a == "--rescore-tdt" && i + 1 < argc) { rescore_w = std::stof(argv[++i]); rescore = true; }
            else if (a == "--spot" && i + 1 < argc) spot.push_back(argv[++i]);
            else if (a == "--spot-file" && i + 1 < argc) {
                std::ifstream f(argv[++i]);
                if (!f) { std::cerr << "Error: cannot open " << argv[i] << "\n"; return 1; }
                for (std::string line; std::getline(f, line);) {
                    while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
                    if (!line.empty()) spot.push_back(line);
                }
            }
            else if (a == "--spot-head" && i + 1 < argc) {
                const std::string hd = argv[++i];
                if (hd != "ctc" && hd != "tdt") { std::cerr << "Unknown spot head: " << hd << "\n"; return 1; }
                spot_tdt = hd == "tdt";
            }
            else if (a == "--spot-hits" && i + 1 < argc) spot_opts.max_hits = std::stoi(argv[++i]);
            else if (a == "--spot-min-score" && i + 1 < argc) spot_opts.min_score = std::stof(argv[++i]);
            else if (a == "--prune" && i + 1 < argc) prune = std::stoi(argv[++i]);
            else if (a == "--lm" && i + 1 < argc) lm_path = argv[++i];
            else if (a == "--lm-alpha" && i + 1 < argc) lm_opts.alpha = std::stof(argv[++i]);
            else if (a == "--lm-beta" && i + 1 < argc) lm_opts.beta = std::stof(argv[++i]);
            else if (a == "--nlm" && i + 1 < argc) nlm_path = argv[++i];
            else if (a == "--nlm-heads" && i + 1 < argc) nlm_heads = std::stoi(argv[++i]);
            else if (a == "--nlm-bos" && i + 1 < argc) nlm_bos = std::stoi(argv[++i]);
            else if (a == "--nlm-eos" && i + 1 < argc) nlm_eos = std::stoi(argv[++i]);
            else if (a == "--nlm-alpha" && i + 1 < argc) nlm_opts.alpha = std::stof(argv[++i]);
            else if (a == "--nlm-beta" && i + 1 < argc) nlm_opts.beta = std::stof(argv[++i]);
            else if (a == "--device-resample") device_resample = true;
            else if (a == "--vad") vad = true;
            else if (a == "--vad-max-piece" && i + 1 < argc) vad_max_piece = std::stof(argv[++i]);
            else if (a == "--gpu" || a == "--streaming") {}
            else if (a == "--timestamps") timestamps = true;
            else if (a == "--latency" && i + 1 < argc) latency = std::stoi(argv[++i]);
            else if (a == "--vocab" && i + 1 < argc) vocab = argv[++i];
            else if (a == "--sortformer-weights" && i + 1 < argc) sf_weights = argv[++i];
            else if (a == "--boost" && i + 1 < argc) boost.push_back(argv[++i]);
            else if (a == "--boost-score" && i + 1 < argc) boost_score = std::stof(argv[++i]);
            else if (a == "--features") { std::cerr << "Error: --features is not supported by this build\n"; return 1; }
            else { std::cerr << "Unknown option: " << a << "\n"; usage(argv[0]); return 1; }
        }
        TranscribeOptions opts;
        opts.decoder = use_ctc ? Decoder::CTC : Decoder::TDT;
        opts.timestamps = timestamps;
        opts.boost_phrases = boost;
        opts.boost_score = boost_score;
        opts.vad = vad;
        opts.vad_max_piece_s = vad_max_piece;
        if (vad && model != "tdt-ctc-110m" && model != "tdt-600m") { std::cerr << "Error: --vad needs --model tdt-ctc-110m or tdt-600m\n"; return 1; }
        if (vad && device_resample) { std::cerr << "Error: --vad works on 16 kHz audio; it does not combine with --device-resample\n"; return 1; }
        if (align && model != "tdt-ctc-110m" && model != "tdt-600m") { std::cerr << "Error: --align needs --model tdt-ctc-110m or tdt-600m\n"; return 1; }
        if (align && vocab.empty()) { std::cerr << "Error: --align needs --vocab\n"; return 1; }
        if (score && model != "tdt-ctc-110m" && model != "tdt-600m") { std::cerr << "Error: --score needs --model tdt-ctc-110m or tdt-600m\n"; return 1; }
        if (score && vocab.empty()) { std::cerr << "Error: --score needs --vocab\n"; return 1; }
        if (!spot.empty() && !spot_tdt && model != "tdt-ctc-110m") {
            std::cerr << "Error: --spot needs a model with a CTC head (--model tdt-ctc-110m), or --spot-head tdt\n";
            return 1;
        }
        if (!spot.empty() && spot_tdt && model != "tdt-ctc-110m" && model != "tdt-600m") { std::cerr << "Error: --spot-head tdt needs --model tdt-ctc-110m or tdt-600m\n"; return 1; }
        if (!spot.empty() && vocab.empty()) { std::cerr << "Error: --spot needs --vocab\n"; return 1; }
        if (rescore && !nbest_given) { std::cerr << "Error: --rescore-tdt needs --nbest N\n"; return 1; }
        if (rescore && model != "tdt-ctc-110m") { std::cerr << "Error: --rescore-tdt needs a model with both heads (--model tdt-ctc-110m)\n"; return 1; }
        if (!lm_path.empty() && (beam <= 0 || rescore || (beam_tdt ? model != "tdt-ctc-110m" && model != "tdt-600m" : model != "tdt-ctc-110m"))) {
            std::cerr << "Error: --lm needs --beam W with the CTC head of --model tdt-ctc-110m, or --beam W --beam-head tdt with --model tdt-ctc-110m or "
                         "tdt-600m (no --rescore-tdt)\n";
            return 1;
        }
        if (!nlm_path.empty() && (beam <= 0 || rescore || !lm_path.empty() || nlm_heads <= 0 || nlm_bos < 0 ||
                                  (beam_tdt ? model != "tdt-ctc-110m" && model != "tdt-600m" : model != "tdt-ctc-110m"))) {
            std::cerr << "Error: --nlm needs --nlm-heads H, --nlm-bos ID and --beam W with the CTC head of --model tdt-ctc-110m, or --beam W --beam-head tdt "
                         "with --model tdt-ctc-110m or tdt-600m (no --rescore-tdt, no --lm)\n";
            return 1;
        }
        if (beam_tdt && beam <= 0) { std::cerr << "Error: --beam-head needs --beam W\n"; return 1; }
        if (beam_tdt && !boost.empty()) { std::cerr << "Error: --beam has no phrase-boosted variant\n"; return 1; }
        // --beam W --beam-head tdt: the TDT beam search's N best hypotheses, each with its path log-probability
        auto print_tdt_beam = [&](const std::vector<ScoredResult> &hyps, double ms) {
            std::cout << "Beam search (tdt): width " << beam << ", " << hyps.size() << " hypotheses\n";
            for (size_t j = 0; j < hyps.size(); ++j) {
                std::cout << "\n=== Hypothesis " << j << " score " << std::setprecision(9) << std::defaultfloat << hyps[j].score << " ===\n";
                print_result(hyps[j].result, timestamps, ms);
            }
            return 0;
        };
        TdtBeamOptions tbo;
        tbo.beam_width = beam; tbo.n_best = nbest; tbo.timestamps = timestamps;
        // ... with --lm: the fused search, lists in fused order, the acoustic and the LM score of every hypothesis
        auto print_tdt_beam_lm = [&](const LanguageModel &lm, const std::vector<LmScoredResult> &hyps, double ms) {
            std::cout << "Beam search (tdt): width " << beam << ", " << lm.order() << "-gram model (" << lm.num_ngrams() << " n-grams), alpha "
                      << std::defaultfloat << lm_opts.alpha << " beta " << lm_opts.beta << ", " << hyps.size() << " hypotheses\n";
            for (size_t j = 0; j < hyps.size(); ++j) {
                std::cout << "\n=== Hypothesis " << j << " score " << std::setprecision(9) << std::defaultfloat << hyps[j].score << " lm " << hyps[j].lm_score
                          << " ===\n";
                print_result(hyps[j].result, timestamps, ms);
            }
            return 0;
        };
        // ... with --nlm: either search's list re-ranked by a Transformer LM, the combined score and both parts of every hypothesis
        auto print_beam_nlm = [&](const char *head, const NeuralLanguageModel &nlm, const std::vector<NlmScoredResult> &hyps, double ms) {
            const pk_nlm_config &c = nlm.config();
            std::cout << "Beam search (" << head << "): width " << beam << ", re-ranked by a Transformer LM (" << c.transformer.num_layers << " layers, d "
                      << c.transformer.hidden_size << ", vocabulary " << c.vocab_size << "), alpha " << std::defaultfloat << nlm_opts.alpha << " beta "
                      << nlm_opts.beta << ", " << hyps.size() << " hypotheses\n";
            for (size_t j = 0; j < hyps.size(); ++j) {
                std::cout << "\n=== Hypothesis " << j << " score " << std::setprecision(9) << std::defaultfloat << hyps[j].score << " am " << hyps[j].am_score
                          << " nlm " << hyps[j].nlm_score << " ===\n";
                print_result(hyps[j].result, timestamps, ms);
            }
            return 0;
        };
        std::cout << "Loading model: " << model << std::endl;
        if (model == "tdt-ctc-110m") {
            Transcriber t(weights, vocab);
            t.to_gpu();
            t.set_device_resampling(device_resample);
            if (align) return run_align(t, audio_path, align_text, align_tdt);
            if (score) return run_score(t, audio_path, score_text);
            if (!spot.empty()) return run_spot(t, audio_path, spot, spot_opts, spot_tdt);
            if (rescore) {                                          // the beam's list re-ranked by the TDT head; --beam W optional (default 8)
                if (!boost.empty()) { std::cerr << "Error: --beam has no phrase-boosted variant\n"; return 1; }
                BeamOptions bo;
                bo.beam_width = beam > 0 ? beam : std::max(8, nbest); bo.n_best = nbest; bo.token_prune = prune;
                RescoreOptions ro;
                ro.tdt_weight = rescore_w;
                const auto hyps = t.transcribe_nbest(audio_path, bo, ro);
                std::cout << "Rescored beam search: width " << bo.beam_width << ", TDT weight " << std::defaultfloat << rescore_w << ", " << hyps.size() << " hypotheses\n";
                for (size_t j = 0; j < hyps.size(); ++j)
                    std::cout << "#" << j + 1 << " [" << std::fixed << std::setprecision(4) << hyps[j].score << "] ctc " << hyps[j].ctc_score << " tdt "
                              << hyps[j].tdt_total << " " << hyps[j].result.text << "\n";
                return 0;
            }
            if (!boost.empty()) std::cout << "Phrase boost: " << boost.size() << " phrases\n";
            if (beam > 0 && beam_tdt) {
                if (!nlm_path.empty()) {
                    const NeuralLanguageModel nlm(nlm_path, nlm_heads, nlm_bos, nlm_eos);
                    const auto t0 = Clock::now();
                    const auto hyps = t.transcribe_nbest_tdt(audio_path, tbo, nlm, nlm_opts);
                    return print_beam_nlm("tdt", nlm, hyps, std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
                }
                if (!lm_path.empty()) {
                    const LanguageModel lm(lm_path);
                    const auto t0 = Clock::now();
                    const auto hyps = t.transcribe_nbest_tdt(audio_path, tbo, lm, lm_opts);
                    return print_tdt_beam_lm(lm, hyps, std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
                }
                const auto t0 = Clock::now();
                const auto hyps = t.transcribe_nbest_tdt(audio_path, tbo);
                return print_tdt_beam(hyps, std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
            }
            if (beam > 0) {
                if (!use_ctc) { std::cerr << "Error: --beam needs the CTC decoder (--ctc / --decoder ctc)\n"; return 1; }
                if (!boost.empty()) { std::cerr << "Error: --beam has no phrase-boosted variant\n"; return 1; }
                BeamOptions bo;
                bo.beam_width = beam; bo.n_best = nbest; bo.token_prune = prune; bo.timestamps = timestamps;
                if (!nlm_path.empty()) {
                    const NeuralLanguageModel nlm(nlm_path, nlm_heads, nlm_bos, nlm_eos);
                    const auto t0 = Clock::now();
                    const auto hyps = t.transcribe_nbest(audio_path, bo, nlm, nlm_opts);
                    return print_beam_nlm("ctc", nlm, hyps, std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
                }
                if (!lm_path.empty()) {                              // shallow fusion: the lists come back in fused order, both parts printed
                    const LanguageModel lm(lm_path);
                    const auto t0 = Clock::now();
                    const auto hyps = t.transcribe_nbest(audio_path, bo, lm, lm_opts);
                    const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
                    std::cout << "Beam search: width " << beam << ", " << lm.order() << "-gram model (" << lm.num_ngrams() << " n-grams), alpha "
                              << std::defaultfloat << lm_opts.alpha << " beta " << lm_opts.beta << ", " << hyps.size() << " hypotheses\n";
                    for (size_t j = 0; j < hyps.size(); ++j) {
                        std::cout << "\n=== Hypothesis " << j << " score " << std::setprecision(9) << std::defaultfloat << hyps[j].score << " lm "
                                  << hyps[j].lm_score << " ===\n";
                        print_result(hyps[j].result, timestamps, ms);
                    }
                    return 0;
                }
                const auto t0 = Clock::now();
                const auto hyps = t.transcribe_nbest(audio_path, bo);
                const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
                std::cout << "Beam search: width " << beam << ", " << hyps.size() << " hypotheses\n";
                for (size_t j = 0; j < hyps.size(); ++j) {
                    std::cout << "\n=== Hypothesis " << j << " score " << std::setprecision(9) << std::defaultfloat << hyps[j].score << " ===\n";
                    print_result(hyps[j].result, timestamps, ms);
                }
                return 0;
            }
            const auto t0 = Clock::now();
            const auto r = t.transcribe(audio_path, opts);
            print_result(r, timestamps, std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
        } else if (model == "tdt-600m") {
            TDTTranscriber t(weights, vocab);
            t.to_gpu();
            t.set_device_resampling(device_resample);
            if (align) return run_align(t, audio_path, align_text, align_tdt);
            if (score) return run_score(t, audio_path, score_text);
            if (!spot.empty()) return run_spot(t, audio_path, spot, spot_opts, true);
            if (beam > 0) {
                if (!beam_tdt) { std::cerr << "Error: this model has no CTC head: --beam needs --beam-head tdt\n"; return 1; }
                if (!nlm_path.empty()) {
                    const NeuralLanguageModel nlm(nlm_path, nlm_heads, nlm_bos, nlm_eos);
                    const auto t0 = Clock::now();
                    const auto hyps = t.transcribe_nbest(audio_path, tbo, nlm, nlm_opts);
                    return print_beam_nlm("tdt", nlm, hyps, std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
                }
                if (!lm_path.empty()) {
                    const LanguageModel lm(lm_path);
                    const auto t0 = Clock::now();
                    const auto hyps = t.transcribe_nbest(audio_path, tbo, lm, lm_opts);
                    return print_tdt_beam_lm(lm, hyps, std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
                }
                const auto t0 = Clock::now();
                const auto hyps = t.transcribe_nbest(audio_path, tbo);
                return print_tdt_beam(hyps, std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
            }
            const auto t0 = Clock::now();
            const auto r = t.transcribe(audio_path, opts);
            print_result(r, timestamps, std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
        } else if (model == "rnnt-600m") {                          // run_rnnt_600m (main.cpp:296-376): ParakeetRNNT + rnnt_greedy_decode
            pk_config cfg;
            detail::check(pk_config_preset("rnnt-600m", &cfg));
            pk_model *m = nullptr;
            detail::check(pk_model_load(weights.c_str(), vocab.empty() ? nullptr : vocab.c_str(), &cfg, &m));
            struct Free { pk_model *m; ~Free() { pk_model_free(m); } } guard{m};
            detail::check(pk_model_to_gpu(m, 0));
            const auto audio = read_audio(audio_path);
            const int64_t off[2] = {0, (int64_t)audio.samples.size()};
            pk_options o{};
            o.decoder = PK_DECODER_TDT;                             // the joint loop; the rnnt_head flag of the preset selects rnnt_greedy_decode
            o.timestamps = timestamps ? 1 : 0;
            pk_result *res = nullptr;
            const auto t0 = Clock::now();
            detail::check(pk_transcribe_pcm(m, audio.samples.data(), off, 1, &o, &res));
            TranscribeResult r;
            r.text = res[0].text ? res[0].text : "";
            r.token_ids.assign(res[0].token_ids, res[0].token_ids + res[0].n_tokens);
            for (int i = 0; i < res[0].n_words; ++i) r.word_timestamps.push_back({res[0].words[i].word, res[0].words[i].start, res[0].words[i].end, res[0].words[i].confidence});
            pk_results_free(res, 1);
            print_result(r, timestamps, std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
        } else if (model == "eou-120m") {
            StreamingTranscriber t(weights, vocab);
            return run_stream(t, audio_path, timestamps);
        } else if (model == "nemotron-600m") {
            NemotronTranscriber t(weights, vocab, make_nemotron_600m_config(latency));
            return run_stream(t, audio_path, timestamps);
        } else if (model == "sortformer") {
            Sortformer sf(weights);
            sf.to_gpu();
            const auto audio = read_audio(audio_path);
            const auto t0 = Clock::now();
            const auto segs = sf.diarize_pcm(audio.samples.data(), audio.samples.size());
            std::cout << "Diarization: " << std::fixed << std::setprecision(1) << std::chrono::duration<double, std::milli>(Clock::now() - t0).count() << " ms\n";
            std::cout << "\n--- Speaker Segments (" << segs.size() << " segments) ---\n";
            for (const auto &s : segs) std::cout << "  Speaker " << s.speaker_id << ": [" << std::fixed << std::setprecision(2) << s.start << "s - " << s.end << "s]\n";
        } else if (model == "diarized") {
            if (sf_weights.empty()) { std::cerr << "Error: --sortformer-weights required for diarized mode\n"; return 1; }
            DiarizedTranscriber dt(weights, sf_weights, vocab);
            dt.to_gpu();
            const auto r = dt.transcribe(audio_path, use_ctc ? Decoder::CTC : Decoder::TDT);
            std::cout << "\n--- Diarized transcription ---\n";
            int cur = -2;
            for (const auto &w : r.words) {
                if (w.speaker_id != cur) { cur = w.speaker_id; std::cout << "\nSpeaker " << cur << ":"; }
                std::cout << ' ' << w.word;
            }
            std::cout << "\n";
        } else {
            std::cerr << "Unknown model type: " << model << "\n";
            usage(argv[0]);
            return 1;
        }
    } catch (const std::exception &e) {
        std::cerr << "Error: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
