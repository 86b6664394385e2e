// bppretrain_main.cc -- BPpretrain_RBM: the first stage of the reference's pipeline, which the reference does not ship
// (its finetune.pl starts from ./pretraining_weights/...wts).  Greedy layer-wise pre-training of a sigmoid net by one-step
// contrastive divergence (csrc/rbm_rule.h): a Gaussian-Bernoulli RBM on layer 1, Bernoulli-Bernoulli RBMs above it, each
// trained for rbm_epochs passes over the training sentences with the layers below it fixed.  The command line is the
// trainer's key=value vocabulary, the host IO is the trainer's (trainer_io: pfiles, norm file, context windows, chunk
// planner, the seeded shuffle: one lrand48 stream, the chunk order of a pass first, then one shuffle per chunk read),
// and the .wts it writes is what BPtrain_Sigmoid initwts_file= reads.
//
//   BPpretrain_RBM fea_file=... targ_file=... norm_file=... fea_dim=257 fea_context=7 train_sent_range=0-7 traincache=102400
//                  init_randem_seed=1 numlayers=5 layersizes=1799,2048,2048,2048,257 bunchsize=128 gpu_used=0
//                  initwts_file=rand.wts outwts_file=pre.wts log_file=pre.log
//                  rbm_epochs=10 rbm_lrate_gauss=0.001 rbm_lrate=0.01 momentum=0.5 weightcost=0.0002 [rbm_layers=1,2,3]
//
// Also accepted: train_pfile_name= for fea_file=, train_cache_frames= for traincache=, train_cache_seed= for
// init_randem_seed=.  targ_file= is read by the trainer's reader (its sentence table must match) and not used; cv_sent_range,
// lrate, MLflag and the other trainer keys are accepted and ignored, so a finetune.pl command line with the rbm_ keys
// added runs as it is.  rbm_layers defaults to every hidden layer, bottom up.  The default rates above are a choice of
// this project, not a measured optimum.  One log line per layer and epoch: the mean reconstruction error per frame.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mlggd.h"
#include "trainer_io.h"

using mlggd_host::Interface;
using mlggd_host::IoError;
using mlggd_host::WorkPara;

namespace {

void chk(int rc, const char *what) {
    if (rc != MLGGD_OK) throw IoError(std::string(what) + " failed: " + mlggd_last_error());
}

struct RbmArgs {
    int epochs = 10;
    float lrate_gauss = 0.001f, lrate = 0.01f;
    std::vector<int> layers;
    bool momentum_given = false, weightcost_given = false;
};

}  // namespace

int main(int argc, char *argv[]) {
    RbmArgs ra;
    std::vector<std::string> args;  // the trainer's own keys, aliases renamed
    for (int a = 1; a < argc; a++) {
        const std::string arg(argv[a]);
        const size_t eq = arg.find('=');
        const std::string key = arg.substr(0, eq), val = eq == std::string::npos ? "" : arg.substr(eq + 1);
        if (key == "rbm_epochs") ra.epochs = atoi(val.c_str());
        else if (key == "rbm_lrate_gauss") ra.lrate_gauss = (float)atof(val.c_str());
        else if (key == "rbm_lrate") ra.lrate = (float)atof(val.c_str());
        else if (key == "rbm_layers") {
            for (size_t pos = 0; pos <= val.size();) {
                const size_t comma = val.find(',', pos);
                ra.layers.push_back(atoi(val.substr(pos, comma == std::string::npos ? comma : comma - pos).c_str()));
                if (comma == std::string::npos) break;
                pos = comma + 1;
            }
        } else if (key == "train_pfile_name") args.push_back("fea_file=" + val);
        else if (key == "train_cache_frames") args.push_back("traincache=" + val);
        else if (key == "train_cache_seed") args.push_back("init_randem_seed=" + val);
        else {
            if (key == "momentum") ra.momentum_given = true;
            if (key == "weightcost") ra.weightcost_given = true;
            args.push_back(arg);
        }
    }
    std::vector<char *> av;
    av.push_back(argv[0]);
    for (std::string &s : args) av.push_back(&s[0]);

    Interface *io = new Interface;
    mlggd_handle eng = nullptr;
    mlggd_rbm_handle rbm = nullptr;
    int status = 0;
    try {
        io->Initial((int)av.size(), av.data(), /*open_output=*/true);
        WorkPara *p = io->para;
        const int L = io->numlayers;
        const float momentum = ra.momentum_given ? p->momentum : 0.5f;
        const float weightcost = ra.weightcost_given ? p->weightcost : 0.0002f;
        if (ra.epochs < 1) throw IoError("rbm_epochs must be positive");
        if (ra.layers.empty())
            for (int l = 1; l <= L - 2; l++) ra.layers.push_back(l);
        for (int l : ra.layers)
            if (l < 1 || l > L - 2)
                throw IoError("rbm_layers: layer " + std::to_string(l) + " is not a hidden layer 1.." + std::to_string(L - 2));
        io->get_pfile_info();
        io->get_chunk_info(p->train_sent_range);
        io->reserve_frame_buffers(io->train_plan);

        mlggd_config cfg;
        memset(&cfg, 0, sizeof(cfg));
        cfg.struct_size = sizeof(cfg);
        cfg.random_seed = p->init_randem_seed;
        cfg.device = p->gpu_used;
        cfg.numlayers = L;
        for (int i = 0; i < L; i++) cfg.layersizes[i] = p->layersizes[i];
        cfg.bunchsize = p->bunchsize;
        cfg.lrate = p->lrate, cfg.momentum = p->momentum, cfg.weightcost = p->weightcost;  // fine-tuning's: not read here
        cfg.shapefactor = 2.0f, cfg.MLflag = 0;
        cfg.max_cache_frames = p->traincache;
        chk(mlggd_create(&cfg, p->weights, p->bias, &eng), "mlggd_create");
        printf("BPpretrain_RBM: %d layers, bunchsize %d, %d epoch(s) per layer, momentum %g, weightcost %g\n", L, p->bunchsize,
               ra.epochs, (double)momentum, (double)weightcost);

        io->chunk_index.resize(io->total_chunks);
        for (int l : ra.layers) {
            const bool gauss = l == 1;
            chk(mlggd_rbm_open(eng, l, gauss ? MLGGD_RBM_GAUSSIAN : MLGGD_RBM_BERNOULLI, gauss ? ra.lrate_gauss : ra.lrate,
                               momentum, weightcost, (uint32_t)p->init_randem_seed, &rbm),
                "mlggd_rbm_open");
            for (int ep = 1; ep <= ra.epochs; ep++) {
                for (unsigned i = 0; i < io->total_chunks; i++) io->chunk_index[i] = (int)i;
                io->GetRandIndex(io->chunk_index.data(), (int)io->total_chunks);
                double sq = 0.0;
                long long frames = 0;
                for (unsigned i = 0; i < io->total_chunks; i++) {
                    const int n = io->Readchunk_frames(io->chunk_index[i]);
                    int steps = 0;
                    double part = 0.0;
                    chk(mlggd_rbm_train_frames(rbm, p->chunk_frames[0], p->fea_context, p->frames_in[0], n, p->first_frame[0],
                                               &steps, &part),
                        "mlggd_rbm_train_frames");
                    sq += part;
                    frames += (long long)steps * p->bunchsize;
                }
                const double mean = frames > 0 ? sq / (double)frames : 0.0;
                io->logf("RBM layer %d (%s) epoch %d of %d: mean reconstruction error per frame %.6f over %lld frames\n", l,
                         gauss ? "gaussian" : "bernoulli", ep, ra.epochs, mean, frames);
                printf("RBM layer %d (%s) epoch %d of %d: mean reconstruction error per frame %.6f over %lld frames\n", l,
                       gauss ? "gaussian" : "bernoulli", ep, ra.epochs, mean, frames);
                if (io->fp_log) fflush(io->fp_log);
            }
            chk(mlggd_rbm_close(rbm), "mlggd_rbm_close");
            rbm = nullptr;
        }
        chk(mlggd_get_weights(eng, p->weights, p->bias), "mlggd_get_weights");
        io->Writeweights();
        printf("all finish!\n");
    } catch (const std::exception &e) {
        io->logf("%s\n", e.what());
        if (io->fp_log) fflush(io->fp_log);
        fprintf(stderr, "%s\n", e.what());
        status = 1;
    }
    if (rbm) mlggd_rbm_close(rbm);
    if (eng) mlggd_destroy(eng);
    delete io;
    return status;
}
