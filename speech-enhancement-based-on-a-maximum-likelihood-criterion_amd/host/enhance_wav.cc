// enhance_wav.cc -- the whole of the original project's decoder (Test_code/decode.m) in one process: noisy RIFF
// WAV -> LPS -> z-normalise with the training norm file -> edge-replicated context of fea_context frames -> sigmoid
// MLP from the trainer's .wts -> de-normalise -> overlap-add resynthesis with the noisy phase -> enhanced RIFF WAV,
// all on the GPU.  With a clean wave and an info file, the quality report of LPS2Wav_be against the clean wave (its
// LPS is the de-normalised network output).
//
//   enhance_wav wts=mlp.wts norm_file=train_noisy.norm (in=noisy.wav out=enhanced.wav | scp=LIST)
//               [fea_context=7] [gpu_used=0] [bunchsize=512] [batch_s=300] [clean=clean.wav info=info.txt]
//               [score=host|device [stoi=1]] [live=BLOCK [sessions=64]] [activation=sigmoid|relu] [nat=T]
//               [gv=FILE [gv_mode=bin|shared]] [mask=select|off [mask_lo=0.25] [mask_hi=0.75] [mask_scale=1]]
//
// mask=: the net is a multi-objective one (csrc/mask_rule.h): its last layer has 2 x bins units, the clean LPS and a
// ratio mask trained with scale mask_scale; the .wts file does not say how it was trained.  select: per bin the mask
// divided by mask_scale picks the noisy LPS (> mask_hi), the mean of noisy LPS and estimate (mask_lo .. mask_hi) or the
// estimate; off: the LPS half alone is decoded.  The defaults are a choice, not a measured optimum.  In every mode but
// live=; the reports are those of the post-filtered rows; gv= still holds one factor per bin.  Without mask= a net
// whose last layer is 2 x bins wide is refused like any other net of the wrong width.
// gv=FILE: global variance equalisation (csrc/gv_rule.h): the normalised network output of bin k is multiplied by the
// factor FILE holds for it -- a plain list or the file an epoch with MLGGD_GVFILE=FILE wrote -- before it is
// de-normalised, in every mode (mlggd_set_gv); gv_mode=shared takes the file's one factor for all bins.  A .wts file
// does not say how it is to be post-filtered.  The reports are those of the equalised rows.
// activation: the hidden units the net was trained with (BPtrain_Sigmoid / BPtrain_ReLU); the .wts file does not say.
// nat=T: the net was trained noise-aware (csrc/nat_rule.h): its input rows end in the mean of the utterance's first T
// normalised frames, layersizes[0] = (fea_context + 1) x bins; the .wts file does not say that either.  Not with live=.
// scp lists "in out" or "in out clean info" lines.  A list is decoded in batches of batch_s seconds of audio by
// mlggd_enhance_waves: the utterances of a batch form one frame stream, so the forward bunches are full, and the
// quality report takes the network's output rows from the same pass.  A batch ends early where the sample rate
// changes.  batch_s=0: one mlggd_enhance_wave call per line.  The files and the lines on stdout are the same either
// way.  Device memory per 16 kHz frame (256 new samples): 512 B wave + 1028 B LPS + 2056 B spectrum + 2048 B time block
// + 512 B output + 1028 B report rows, an eighth of headroom on each, and 5 x 1028 B of frame stream and network output
// = about 13 KB; 62.5 frames per second make 0.8 MB per second of audio, 250 MB at the default batch_s=300.
//
// score=host (the default): the report is formed in double on the host, one utterance after the other.  score=device:
// mlggd_enhance_waves_scored forms it in fp32 on the GPU from the buffers of the decoding pass (a single pair and
// batch_s=0 lines as batches of one), over the frames the clean wave has; the clean waves are read before the pass, and
// a list ends with one line: the number of scored utterances and their mean segmental SNR and LSD.  The enhanced waves
// are the same bytes either way; it adds 512 B clean wave + 2056 B clean spectrum + 12 B per frame to the figures above.
// stoi=1 (with score=device): mlggd_enhance_waves_scored_stoi also forms the STOI of every scored utterance's enhanced
// int16 wave against its clean wave, over the samples both the clean and the noisy wave have: the utterance's line on
// stdout ends with " stoi=V" (nan: too short or silent for a value) and the last line with the mean over the utterances
// that have a value and their number.  Files and the other lines are the same bytes with and without it.
// live=BLOCK (scp lists of "in out" lines): the utterances are decoded as concurrent live sessions of one group
// (mlggd_live_*): every push feeds BLOCK samples to each of up to `sessions` utterances, an utterance is ended with its
// last block, and its slot is refilled from the list.  The group is reopened where the sample rate changes.  The files
// are byte-identical to the default mode's; the lines on stdout come in the order the utterances finish.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "tool_io.h"

[[noreturn]] void die(const std::string &m) {
    fprintf(stderr, "enhance_wav: %s\n", m.c_str());
    exit(1);
}

struct Job {
    std::string in, out, clean, info;
};

// an utterance read and checked, waiting for its batch
struct Item {
    Job job;
    std::vector<int16_t> noisy;
    int rate = 0, fs = 0, F = 0;
    std::vector<int16_t> clean;  // score=device: the clean wave, and the frames it is scored over
    int Fm = 0;
};

// the clean wave of an utterance and the frames of min(clean, noisy); a wave that cannot be scored goes to `bad`
template <typename Bad>
std::vector<int16_t> read_clean(const Item &it, int *Fm, Bad bad) {
    int L, S, N;
    tool_io::spectral_params(it.fs, &L, &S, &N);
    int cr = 0;
    std::vector<int16_t> cw = tool_io::read_wav(it.job.clean, &cr);
    if (cr != it.rate) bad(it.job.clean + ": sample rate differs from " + it.job.in);
    const int Fc = cw.size() < (size_t)L ? 0 : (int)((cw.size() - (L - S)) / S);
    *Fm = std::min(it.F, Fc);
    if (*Fm == 0) bad(it.job.clean + ": shorter than one frame");
    return cw;
}

// LPS2Wav_be's report for one utterance from its enhanced LPS rows y [F][D]
void report(const Item &it, const float *y) {
    int Fm = 0;
    const std::vector<int16_t> cw = read_clean(it, &Fm, die);
    double segsnr = 0.0, lsd = 0.0;
    tool_io::quality(it.fs, cw, it.noisy, y, Fm, &segsnr, &lsd);
    tool_io::write_info(it.job.info, segsnr, lsd);
}

int main(int argc, char **argv) {
    std::string wts, norm_file, in, out, scp, clean, info, score = "host", gv, gv_mode = "bin";
    const char *usage =
        "usage: enhance_wav wts=F norm_file=F (in=F out=F | scp=LIST) [fea_context=7] [gpu_used=0] [bunchsize=512] "
        "[batch_s=300] [clean=F info=F] [score=host|device [stoi=1]] [live=BLOCK [sessions=64]] [activation=sigmoid|relu] "
        "[nat=T] [gv=FILE [gv_mode=bin|shared]] [mask=select|off [mask_lo=0.25] [mask_hi=0.75] [mask_scale=1]]";
    tool_io::MaskArg mask;
    int ctx = 7, gpu = 0, bunch = 512, live_block = 0, n_slots = 64, act = MLGGD_ACT_SIGMOID, nat = 0;
    bool live = false, score_given = false, want_stoi = false;
    double batch_s = 300.0;
    for (int a = 1; a < argc; a++) {
        const std::string arg(argv[a]);
        const size_t eq = arg.find('=');
        if (eq == std::string::npos) die("Arg: " + arg + "  Format Error");
        const std::string k = arg.substr(0, eq), v = arg.substr(eq + 1);
        if (k == "wts") wts = v;
        else if (k == "norm_file") norm_file = v;
        else if (k == "in") in = v;
        else if (k == "out") out = v;
        else if (k == "scp") scp = v;
        else if (k == "clean") clean = v;
        else if (k == "info") info = v;
        else if (k == "fea_context") ctx = atoi(v.c_str());
        else if (k == "gpu_used") gpu = atoi(v.c_str());
        else if (k == "bunchsize") bunch = atoi(v.c_str());
        else if (k == "batch_s") batch_s = atof(v.c_str());
        else if (k == "score") score = v, score_given = true;
        else if (k == "stoi") want_stoi = atoi(v.c_str()) != 0;
        else if (k == "live") live_block = atoi(v.c_str()), live = true;
        else if (k == "sessions") n_slots = atoi(v.c_str());
        else if (k == "activation") act = tool_io::parse_activation(v);
        else if (k == "nat") nat = tool_io::parse_nat(v);
        else if (k == "gv") gv = v;
        else if (k == "gv_mode") gv_mode = v;
        else if (k == "mask") mask.mode = tool_io::parse_mask_mode(v), mask.given = true;
        else if (k == "mask_lo") mask.lo = tool_io::parse_mask_value(k, v);
        else if (k == "mask_hi") mask.hi = tool_io::parse_mask_value(k, v);
        else if (k == "mask_scale") mask.scale = tool_io::parse_mask_value(k, v);
        else die("unknown argument " + k);
    }
    if (wts.empty() || norm_file.empty() || (scp.empty() && (in.empty() || out.empty())))
        die(usage);
    if (score != "host" && score != "device") die("score=" + score + ": must be host or device\n" + usage);
    const bool on_device = score == "device";
    if (want_stoi && !on_device) die("stoi=1 needs score=device: STOI is formed on the GPU only\n" + std::string(usage));
    if (ctx < 1 || ctx % 2 == 0) die("fea_context must be odd");
    if (clean.empty() != info.empty()) die("clean= and info= go together");
    if (!clean.empty() && !scp.empty()) die("clean= / info= need a single in= / out= pair (or four-field scp lines)");
    if (batch_s < 0) die("batch_s must not be negative");
    if (live) {
        if (score_given) die("live= and score= do not go together: a live session has no quality report");
        if (scp.empty()) die("live= needs an scp= list");
        if (live_block < 1) die("live= must be a block of at least one sample");
        if (n_slots < 1) die("sessions= must be at least 1");
        if (nat > 0) die("live= and nat= do not go together: a live session of a noise-aware net is not built");
        if (mask.given) die("live= and mask= do not go together: a live session of a mask net is not built");
    }

    const tool_io::Model model = tool_io::read_wts(wts);
    if (mask.given && model.ls.back() % 2 != 0) die("mask=: the last layer is not 2 x the bins (LPS and mask)");
    const int D = mask.given ? model.ls.back() / 2 : model.ls.back();  // the bins of a frame
    if (nat > 0 && model.ls[0] != (ctx + 1) * D) die("layersizes[0] is not (fea_context + 1) x the output dimension (nat=)");
    if (nat == 0 && model.ls[0] != ctx * D) die("layersizes[0] is not fea_context x the output dimension");
    std::vector<float> mean, inv;
    tool_io::read_norm(norm_file, D, mean, inv);
    std::vector<float> eta = tool_io::read_gv_arg(gv, gv_mode, D);  // a bad file ends the run before the engine exists
    mlggd_handle h = tool_io::create_engine(model, gpu, bunch, 0, act, nat, mask.given ? D : 0);
    if (mask.given) {
        if (mlggd_set_mask(h, mask.mode, mask.lo, mask.hi, mask.scale) != MLGGD_OK)
            die(std::string("mlggd_set_mask: ") + mlggd_last_error());
        if (!eta.empty()) eta.resize((size_t)2 * D, 1.0f);  // one factor per output; the decoders read the LPS half's
    }
    if (!eta.empty() && mlggd_set_gv(h, eta.data()) != MLGGD_OK) die(std::string("mlggd_set_gv: ") + mlggd_last_error());

    std::vector<Job> jobs;
    if (!scp.empty()) {
        std::ifstream f(scp);
        if (!f) die("cannot open " + scp);
        std::string line;
        for (int ln = 1; std::getline(f, line); ln++) {
            std::istringstream ss(line);
            std::vector<std::string> w;
            for (std::string t; ss >> t;) w.push_back(t);
            if (w.empty()) continue;
            if (w.size() != 2 && w.size() != 4)
                die(scp + " line " + std::to_string(ln) + ": expected \"in out\" or \"in out clean info\"");
            jobs.push_back(w.size() == 2 ? Job{w[0], w[1], "", ""} : Job{w[0], w[1], w[2], w[3]});
        }
    } else {
        jobs.push_back(Job{in, out, clean, info});
    }
    if (live) {
        // the list as concurrent live sessions: slots refilled as they free up, one group per run of one sample rate
        struct Slot {
            bool busy = false;
            Item it;
            size_t at = 0;
            std::vector<int16_t> out;
        };
        size_t next = 0;
        Item held;
        bool have_held = false;
        auto fetch = [&](Item *it) {  // the next utterance of the list, read and checked
            if (have_held) {
                *it = std::move(held);
                have_held = false;
                return true;
            }
            if (next >= jobs.size()) return false;
            const Job &job = jobs[next++];
            if (!job.clean.empty()) die(job.in + ": live= takes \"in out\" lines only");
            *it = Item();
            it->job = job;
            it->noisy = tool_io::read_wav(job.in, &it->rate);
            it->fs = tool_io::rate_khz(it->rate);
            if (!it->fs) die(job.in + ": sample rate " + std::to_string(it->rate) + " Hz is not 8000, 11000 or 16000");
            int L, S, N;
            tool_io::spectral_params(it->fs, &L, &S, &N);
            if (it->noisy.size() < (size_t)L) die(job.in + ": shorter than one frame");
            it->F = (int)((it->noisy.size() - (L - S)) / S);
            return true;
        };
        for (Item head; fetch(&head);) {  // the head of a run of one rate goes back to be fetched by the first slot
            held = std::move(head);
            have_held = true;
            const int rate = held.rate, fs = held.fs;
            mlggd_live_handle g = nullptr;
            if (mlggd_live_open(h, fs, ctx, mean.data(), inv.data(), n_slots, &g) != MLGGD_OK)
                die(std::string("mlggd_live_open: ") + mlggd_last_error());
            std::vector<Slot> slots(n_slots);
            std::vector<int64_t> off(n_slots + 1), out_off(n_slots + 1), had(n_slots), add(n_slots);
            std::vector<uint8_t> end(n_slots);
            std::vector<int16_t> packed, enh;
            bool more = true;  // the list may still hold utterances of this rate
            for (;;) {
                int busy = 0;
                for (Slot &sl : slots) {
                    if (!sl.busy && more) {
                        Item nx;
                        if (!fetch(&nx)) {
                            more = false;
                        } else if (nx.rate != rate) {
                            held = std::move(nx);
                            have_held = true;
                            more = false;
                        } else {
                            sl.busy = true, sl.it = std::move(nx), sl.at = 0;
                            sl.out.clear();
                        }
                    }
                    busy += sl.busy;
                }
                if (!busy) break;
                packed.clear();
                off[0] = 0;
                for (int u = 0; u < n_slots; u++) {
                    Slot &sl = slots[u];
                    const size_t n = sl.busy ? std::min((size_t)live_block, sl.it.noisy.size() - sl.at) : 0;
                    if (n) packed.insert(packed.end(), sl.it.noisy.begin() + sl.at, sl.it.noisy.begin() + sl.at + n);
                    sl.at += n;
                    add[u] = (int64_t)n;
                    off[u + 1] = off[u] + (int64_t)n;
                    end[u] = sl.busy && sl.at == sl.it.noisy.size();
                }
                if (mlggd_live_received(g, had.data()) != MLGGD_OK ||
                    mlggd_live_layout(fs, ctx, n_slots, had.data(), add.data(), end.data(), out_off.data()) != MLGGD_OK)
                    die(std::string("mlggd_live_layout: ") + mlggd_last_error());
                enh.resize((size_t)out_off[n_slots] + 1);
                if (mlggd_live_push(g, packed.data(), off.data(), end.data(), enh.data(), nullptr, out_off[n_slots],
                                    out_off.data()) != MLGGD_OK)
                    die(std::string("mlggd_live_push: ") + mlggd_last_error());
                for (int u = 0; u < n_slots; u++) {
                    Slot &sl = slots[u];
                    sl.out.insert(sl.out.end(), enh.begin() + out_off[u], enh.begin() + out_off[u + 1]);
                    if (!end[u]) continue;
                    tool_io::write_wav(sl.it.job.out, sl.out.data(), sl.out.size(), sl.it.rate);
                    printf("%s -> %s (%d frames)\n", sl.it.job.in.c_str(), sl.it.job.out.c_str(), sl.it.F);
                    sl.busy = false;
                }
            }
            mlggd_live_close(g);
        }
        mlggd_destroy(h);
        return 0;
    }
    const bool batched = !scp.empty() && batch_s > 0;

    // the batch: utterances of one rate, decoded by one mlggd_enhance_waves call when it is full or the rate changes
    std::vector<Item> pend;
    size_t pend_samples = 0;
    int n_scored = 0, n_stoi = 0;
    double sum_segsnr = 0.0, sum_lsd = 0.0, sum_stoi = 0.0;
    auto flush = [&]() {
        if (pend.empty()) return;
        const int n = (int)pend.size(), fs = pend[0].fs;
        std::vector<int64_t> off(n + 1, 0), out_off(n + 1, 0);
        std::vector<int32_t> frame_off(n + 1, 0);
        for (int u = 0; u < n; u++) off[u + 1] = off[u] + (int64_t)pend[u].noisy.size();
        std::vector<int16_t> packed((size_t)off[n]);
        bool want_lps = false;
        for (int u = 0; u < n; u++) {
            std::copy(pend[u].noisy.begin(), pend[u].noisy.end(), packed.begin() + off[u]);
            want_lps = want_lps || !pend[u].job.clean.empty();
        }
        const bool scored = on_device && want_lps;
        if (scored) want_lps = false;
        if (mlggd_enhance_waves_layout(fs, n, off.data(), frame_off.data(), out_off.data()) != MLGGD_OK)
            die(std::string("mlggd_enhance_waves_layout: ") + mlggd_last_error());
        std::vector<int16_t> enh((size_t)out_off[n]);
        std::vector<float> lps(want_lps ? (size_t)frame_off[n] * D : 0);
        std::vector<float> segsnr(scored ? n : 0), lsd(scored ? n : 0), stoi(scored && want_stoi ? n : 0);
        if (scored) {  // the clean waves in the noisy layout, zero-padded; an utterance without one scores no frame
            std::vector<int16_t> cpacked((size_t)off[n], 0);
            std::vector<int32_t> sframes(n, 0);
            std::vector<int64_t> ssamples(n, 0);
            for (int u = 0; u < n; u++) {
                const std::vector<int16_t> &c = pend[u].clean;
                std::copy(c.begin(), c.begin() + std::min(c.size(), pend[u].noisy.size()), cpacked.begin() + off[u]);
                sframes[u] = pend[u].Fm;
                ssamples[u] = (int64_t)std::min(c.size(), pend[u].noisy.size());
            }
            if (want_stoi) {
                if (mlggd_enhance_waves_scored_stoi(h, fs, ctx, mean.data(), inv.data(), n, packed.data(),
                                                    cpacked.data(), off.data(), sframes.data(), enh.data(), nullptr,
                                                    nullptr, segsnr.data(), lsd.data(), ssamples.data(), stoi.data(),
                                                    nullptr) != MLGGD_OK)
                    die(std::string("mlggd_enhance_waves_scored_stoi: ") + mlggd_last_error());
            } else if (mlggd_enhance_waves_scored(h, fs, ctx, mean.data(), inv.data(), n, packed.data(), cpacked.data(),
                                           off.data(), sframes.data(), enh.data(), nullptr, nullptr, segsnr.data(),
                                           lsd.data()) != MLGGD_OK)
                die(std::string("mlggd_enhance_waves_scored: ") + mlggd_last_error());
        } else if (mlggd_enhance_waves(h, fs, ctx, mean.data(), inv.data(), n, packed.data(), off.data(), enh.data(),
                                       nullptr, want_lps ? lps.data() : nullptr) != MLGGD_OK)
            die(std::string("mlggd_enhance_waves: ") + mlggd_last_error());
        for (int u = 0; u < n; u++) {
            const Item &it = pend[u];
            tool_io::write_wav(it.job.out, enh.data() + out_off[u], (size_t)(out_off[u + 1] - out_off[u]), it.rate);
            printf("%s -> %s (%d frames)", it.job.in.c_str(), it.job.out.c_str(), it.F);
            if (scored && want_stoi && !it.job.clean.empty()) {
                if (std::isnan(stoi[u])) {
                    printf(" stoi=nan");
                } else {
                    printf(" stoi=%f", stoi[u]);
                    n_stoi++;
                    sum_stoi += stoi[u];
                }
            }
            printf("\n");
            if (it.job.clean.empty()) continue;
            if (scored) {
                tool_io::write_info(it.job.info, segsnr[u], lsd[u]);
                n_scored++;
                sum_segsnr += segsnr[u];
                sum_lsd += lsd[u];
            } else {
                report(it, lps.data() + (size_t)frame_off[u] * D);
            }
        }
        pend.clear();
        pend_samples = 0;
    };
    // an utterance that cannot be decoded ends the run after the ones before it have been written
    auto die_in_order = [&](const std::string &m) {
        flush();
        die(m);
    };

    for (const auto &job : jobs) {
        Item it;
        it.job = job;
        it.noisy = tool_io::read_wav(job.in, &it.rate);
        const int rate = it.rate, fs = it.fs = tool_io::rate_khz(rate);
        if (!fs) die_in_order(job.in + ": sample rate " + std::to_string(rate) + " Hz is not 8000, 11000 or 16000");
        int L, S, N;
        tool_io::spectral_params(fs, &L, &S, &N);
        const std::vector<int16_t> &noisy = it.noisy;
        if (noisy.size() < (size_t)L) die_in_order(job.in + ": shorter than one frame");
        const int F = it.F = (int)((noisy.size() - (L - S)) / S);
        if (on_device && !job.clean.empty()) it.clean = read_clean(it, &it.Fm, die_in_order);
        // (a mask net with a host report: the post-filtered rows come from the batch entry, as a batch of one)
        if (batched || on_device || (mask.given && !job.clean.empty())) {
            if (!pend.empty() && pend[0].rate != rate) flush();
            pend_samples += noisy.size();
            pend.push_back(std::move(it));
            if (!batched || (double)pend_samples >= batch_s * rate) flush();
            continue;
        }
        std::vector<int16_t> enh((size_t)F * S + L - S);
        int n_out = 0;
        if (mlggd_enhance_wave(h, fs, ctx, mean.data(), inv.data(), (int)noisy.size(), noisy.data(), enh.data(), nullptr,
                               &n_out) != MLGGD_OK)
            die(std::string("mlggd_enhance_wave: ") + mlggd_last_error());
        tool_io::write_wav(job.out, enh.data(), (size_t)n_out, rate);
        printf("%s -> %s (%d frames)\n", job.in.c_str(), job.out.c_str(), F);
        if (!job.clean.empty()) {
            // the enhanced LPS rows: the same chain through the public pieces (decode.m:31-61)
            std::vector<float> lps((size_t)F * D);
            int Fq = 0;
            if (mlggd_wave_to_lps(gpu, fs, (int)noisy.size(), noisy.data(), &Fq, lps.data()) != MLGGD_OK)
                die(std::string("mlggd_wave_to_lps: ") + mlggd_last_error());
            const int half = (ctx - 1) / 2, np = F + 2 * half;
            std::vector<float> stream((size_t)np * D);
            for (int t = 0; t < np; t++) {
                const int src = std::min(std::max(t - half, 0), F - 1);
                for (int j = 0; j < D; j++) stream[(size_t)t * D + j] = (lps[(size_t)src * D + j] - mean[j]) * inv[j];
            }
            std::vector<int32_t> first(F);
            for (int t = 0; t < F; t++) first[t] = t;
            std::vector<float> y((size_t)F * D);
            if (nat > 0) {  // the noise row from the utterance's own normalised rows (stream rows half .. half + F)
                const int32_t foff[2] = {0, F};
                std::vector<float> z(D);
                std::vector<int32_t> zrow(F, 0);
                if (mlggd_nat_estimate(D, 1, foff, stream.data() + (size_t)half * D, nat, z.data()) != MLGGD_OK ||
                    mlggd_forward_frames_nat(h, np, ctx, stream.data(), F, first.data(), 1, z.data(), zrow.data(),
                                             y.data()) != MLGGD_OK)
                    die(std::string("mlggd_forward_frames_nat: ") + mlggd_last_error());
            } else if (mlggd_forward_frames(h, np, ctx, stream.data(), F, first.data(), y.data()) != MLGGD_OK)
                die(std::string("mlggd_forward_frames: ") + mlggd_last_error());
            for (size_t i = 0; i < y.size(); i++) {  // csrc/gv_rule.h: one rounding per operation
                const float s = eta.empty() ? y[i] : y[i] * eta[i % D];
                const float q = s / inv[i % D];
                y[i] = q + mean[i % D];
            }
            report(it, y.data());
        }
    }
    flush();
    if (on_device && !scp.empty()) {
        if (n_scored) {
            printf("scored %d utterances: mean segmental SNR %f dB, mean LSD %f dB", n_scored, sum_segsnr / n_scored,
                   sum_lsd / n_scored);
            if (want_stoi && n_stoi) printf(", mean STOI %f over %d utterances", sum_stoi / n_stoi, n_stoi);
            else if (want_stoi) printf(", no utterance has a STOI value");
            printf("\n");
        } else {
            printf("scored 0 utterances\n");
        }
    }
    mlggd_destroy(h);
    return 0;
}
