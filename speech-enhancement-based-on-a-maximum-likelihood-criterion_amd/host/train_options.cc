// train_options.cc -- the trainer's environment, read once (train_options.h).  Header-only file readers and the two
// rule headers only: nothing here calls into libmlggd.so.
#include "train_options.h"

#include <cstdio>
#include <cstdlib>

#include "binfile.h"
#include "errmodel.h"
#include "scalefile.h"

namespace mlggd_host {
namespace {

std::string env_str(const EnvLookup &env, const char *name) {
    const char *v = env(name);
    return v ? v : "";
}

int env_int(const EnvLookup &env, const char *name, int dflt) {
    const char *v = env(name);
    return v && *v ? atoi(v) : dflt;
}

void env_float(const EnvLookup &env, const char *name, float *v) {
    const char *t = env(name);
    if (!t || !*t) return;
    char *end = nullptr;
    *v = strtof(t, &end);
    if (end == t || *end != 0) throw IoError(std::string(name) + "=" + t + ": not a number");
}

// VAR=on|off with FILEVAR=PATH beside it: true for `on`, false for `off` or no word; another word, or a file without
// `on`, is refused
bool mode_with_file(const EnvLookup &env, const char *var, const char *on, const char *off, const char *filevar, std::string *fn) {
    const std::string word = env_str(env, var);
    *fn = env_str(env, filevar);
    if (!word.empty() && word != on && word != off) throw IoError(std::string(var) + "=" + word + ": must be " + on + " or " + off);
    if (!fn->empty() && word != on) throw IoError(std::string(filevar) + "=" + *fn + ": needs " + var + "=" + on);
    return word == on;
}

// `what`, e.g. "MLGGD_SCALE=learned: a learned scale needs", is refused on a beta-norm run
void need_ml(const WorkPara &p, const std::string &what) {
    if (p.MLflag != 1) throw IoError(what + " MLflag=1, this run has MLflag=" + std::to_string(p.MLflag));
}

// a state file is optional: the first epoch of a run has none yet
bool exists(const std::string &fn) {
    FILE *fp = fn.empty() ? nullptr : fopen(fn.c_str(), "rb");
    if (fp) fclose(fp);
    return fp != nullptr;
}

// one value per output bin from the file VAR names (binfile.h); empty without the variable
std::vector<float> per_bin(const char *var, const std::string &fn, const char *needs, const WorkPara &p, int D, float fallback,
                           bool (*parse)(const std::string &, int, float, float *, std::string *)) {
    std::vector<float> v;
    if (fn.empty()) return v;
    need_ml(p, std::string(var) + "=" + fn + ": " + needs);
    v.resize(D);
    std::string why;
    if (!parse(fn, D, fallback, v.data(), &why)) throw IoError(std::string(var) + ": " + why);
    return v;
}

}  // namespace

LaunchEnv read_launch_env(const EnvLookup &env) {
    LaunchEnv l;
    l.world = env_int(env, "WORLD_SIZE", 1);
    l.rank = env_int(env, "RANK", 0);
    l.local_rank = env_int(env, "LOCAL_RANK", l.rank);
    l.timing = env("MLGGD_TIMING") != nullptr;
    return l;
}

TrainOptions read_train_options(const WorkPara &p, int numlayers, const EnvLookup &env) {
    TrainOptions o;
    static_cast<LaunchEnv &>(o) = read_launch_env(env);
    const int D = p.layersizes[numlayers - 1];
    o.frames = env_int(env, "MLGGD_EXPANDED", 0) == 0;
    o.pinned = env_int(env, "MLGGD_PINNED", 1) != 0;
    o.watchdog_s = env_int(env, "MLGGD_WATCHDOG_S", 900);
    o.id_file = env_str(env, "MLGGD_ID_FILE");
    o.rendezvous_timeout = env_int(env, "MLGGD_RENDEZVOUS_TIMEOUT", 600);

    o.errmodel_fn = env_str(env, "MLGGD_ERRMODEL");
    o.asymmodel_fn = env_str(env, "MLGGD_ASYMMODEL");
    o.gv_fn = env_str(env, "MLGGD_GVFILE");
    const char *grid = env("MLGGD_ERRMODEL_BETAS");
    if (!o.errmodel_fn.empty() && o.rank == 0) o.model_betas = beta_grid(grid);
    o.shapes_fn = env_str(env, "MLGGD_SHAPEFACTORS");
    o.shapes = per_bin("MLGGD_SHAPEFACTORS", o.shapes_fn, "per-bin shape factors need", p, D, p.shapefactor, parse_shapefactors);
    // the asymmetric model alone: its bad grid is reported here, behind the shapes (beta_grid returns at least one
    // shape or throws, so an empty grid means that it has not been parsed yet)
    if (!o.asymmodel_fn.empty() && o.rank == 0 && o.model_betas.empty()) o.model_betas = beta_grid(grid);
    o.asym_fn = env_str(env, "MLGGD_ASYMMETRY");
    o.skews = per_bin("MLGGD_ASYMMETRY", o.asym_fn, "a skew per bin needs", p, D, 1.0f, parse_asymmetry);

    o.scale_learned = mode_with_file(env, "MLGGD_SCALE", "learned", "alternating", "MLGGD_SCALE_FILE", &o.scale_fn);
    if (o.scale_learned) {
        need_ml(p, "MLGGD_SCALE=learned: a learned scale needs");
        env_float(env, "MLGGD_SCALE_LRATE", &o.scale_lrate);
        env_float(env, "MLGGD_SCALE_MOMENTUM", &o.scale_momentum);
        env_float(env, "MLGGD_SCALE_VMAX", &o.scale_vmax);
        if (!scale_rule::valid(scale_rule::kLearned, o.scale_lrate, o.scale_momentum, o.scale_vmax))
            throw IoError("MLGGD_SCALE=learned: MLGGD_SCALE_LRATE must be finite and >= 0, MLGGD_SCALE_MOMENTUM in [0, 1), "
                          "MLGGD_SCALE_VMAX finite and > 0");
        if (exists(o.scale_fn)) {
            o.scale_alpha.resize(D);
            o.scale_velocity.resize(D);
            std::string why;
            if (!parse_scale_state(o.scale_fn, D, o.scale_alpha.data(), o.scale_velocity.data(), &why, &o.scale_steps0))
                throw IoError("MLGGD_SCALE_FILE: " + why);
        }
    }

    o.adam = mode_with_file(env, "MLGGD_OPTIMIZER", "adam", "sgd", "MLGGD_OPT_FILE", &o.opt_fn);
    if (o.adam) {
        if (o.world > 1)
            throw IoError("MLGGD_OPTIMIZER=adam: Adam runs on a single rank, this run has WORLD_SIZE=" + std::to_string(o.world));
        env_float(env, "MLGGD_ADAM_BETA1", &o.adam_beta1);
        env_float(env, "MLGGD_ADAM_BETA2", &o.adam_beta2);
        env_float(env, "MLGGD_ADAM_EPS", &o.adam_eps);
        if (!adam_rule::valid(o.adam_beta1, o.adam_beta2, o.adam_eps))
            throw IoError("MLGGD_OPTIMIZER=adam: MLGGD_ADAM_BETA1 and MLGGD_ADAM_BETA2 must lie in [0, 1), MLGGD_ADAM_EPS must be "
                          "finite and > 0");
        if (exists(o.opt_fn)) {
            std::string why;
            if (!read_opt_state(o.opt_fn, p.layersizes, numlayers, &o.opt_state, &why)) throw IoError("MLGGD_OPT_FILE: " + why);
            o.opt_restored = true;
        }
    }
    return o;
}

}  // namespace mlggd_host
