// ssd_abi.hip -- the extern "C" boundary of libssd_hip.so (declared in include/ssd_hip.h).
// Host code only: argument checking, map parsing, device allocation, kernel launches.  No torch types, no
// exceptions across the boundary, nothing aborts; all launches are asynchronous on the caller's stream.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "ssd_device.h"
#include "../../include/ssd_hip_train.h"
#include "../../include/ssd_hip_reward.h"
#include "../../include/ssd_hip_tie.h"
#include "../../include/ssd_hip_mix.h"

using namespace ssd;

struct ssd_env {
    DevSpec hs;        // host copy
    DevSpec* dspec;    // device copy
    DevState st;
    int device;
    int n_spawn;
    uint32_t* beam_rec;   // render mode (ssd_set_render): [N, n] beam record of the last step; null = render mode off
    uint8_t* render_lut;  // render mode: full-colour table by render class (17 x 3 bytes)
    uint8_t host_lut[64];
};

static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, const char* a = "") {
    std::snprintf(g_err, sizeof g_err, fmt, a);
    return code;
}
#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) return fail(SSD_ERR_DEVICE, #expr ": %s", hipGetErrorString(e_)); \
    } while (0)

static uint32_t magic(uint32_t d) { return d <= 1 ? 0xFFFFFFFFu : (uint32_t)(0x100000000ull / d) + 1u; }

extern "C" {

int ssd_abi_version(void) { return SSD_ABI_VERSION; }
const char* ssd_last_error(void) { return g_err; }

// `u < p` for the COUNTER-mode draw u = m * 2^-24 (24-bit integer m): p * 2^24 is an exact fp64 scaling, so u < p  <=>  m < ceil(p * 2^24)
static uint32_t draw_threshold(double p) { return p >= 1.0 ? (1u << 24) : !(p > 0.0) ? 0u : (uint32_t)std::ceil(p * 16777216.0); }

int ssd_create(const ssd_config* cfg, ssd_env** out) {
    if (!cfg || !out || !cfg->ascii_map) return fail(SSD_ERR_INVALID, "null argument");
    if (cfg->n_agents < 1 || cfg->n_agents > SSD_MAX_AGENTS) return fail(SSD_ERR_INVALID, "n_agents out of range (1..10)");
    if (cfg->height < 3 || cfg->width < 3 || cfg->height > 255 || cfg->width > 255 || cfg->height * cfg->width > SSD_MAX_CELLS)
        return fail(SSD_ERR_INVALID, "map size out of range");
    if (cfg->n_env < 1) return fail(SSD_ERR_INVALID, "n_env must be >= 1");
    if (cfg->view_size < 0 || cfg->view_size > 31) return fail(SSD_ERR_INVALID, "view_size out of range (0..31)");
    {   // LDS budget: 4 waves (envs) per workgroup must fit the 160 KiB of a CU
        const long V = 2L * cfg->view_size + 1, pm = (cfg->height + 2L * cfg->view_size) * (cfg->width + 2L * cfg->view_size);
        const long per_wave = 2L * ((cfg->height * cfg->width + 15) & ~15) + pm + 16 + cfg->n_agents * 3L * V * V + 32 + 64 + (cfg->n_agents * SSD_CODE_AGENT_STRIDE(V) <= 2560 ? cfg->n_agents : 1) * SSD_CODE_AGENT_STRIDE(V) + 16;
        if (per_wave * 4 > 160 * 1024) return fail(SSD_ERR_INVALID, "map / view_size / n_agents exceed the LDS budget of one workgroup");
    }
    if (cfg->spawn_rotation > 3) return fail(SSD_ERR_INVALID, "spawn_rotation must be -1..3");
    if (cfg->env_kind != SSD_ENV_CLEANUP && cfg->env_kind != SSD_ENV_HARVEST) return fail(SSD_ERR_INVALID, "env_kind");
    if (cfg->rng_mode != SSD_RNG_TAPE && cfg->rng_mode != SSD_RNG_COUNTER) return fail(SSD_ERR_INVALID, "rng_mode");

    ssd_env* E = new (std::nothrow) ssd_env();
    if (!E) return fail(SSD_ERR_NOMEM, "host allocation failed");
    std::memset(E, 0, sizeof *E);
    DevSpec& S = E->hs;
    S.kind = cfg->env_kind; S.H = cfg->height; S.W = cfg->width; S.HW = S.H * S.W; S.GS = (S.HW + 15) & ~15;
    S.n = cfg->n_agents; S.N = cfg->n_env; S.v = cfg->view_size; S.V = 2 * S.v + 1; S.VV = S.V * S.V; S.VVp = (S.VV + 3) & ~3;
    S.Wp = S.W + 2 * S.v; S.PMS = ((S.H + 2 * S.v) * S.Wp + 15) & ~15;
    S.vshift = 0; while ((1 << S.vshift) < S.V) ++S.vshift;
    S.episode_limit = cfg->episode_limit; S.spawn_rotation = cfg->spawn_rotation < 0 ? -1 : cfg->spawn_rotation;
    S.obs_color = cfg->obs_color == SSD_COLOR_FULL ? SSD_COLOR_FULL : SSD_COLOR_SIMPLIFIED;
    S.rng_mode = cfg->rng_mode; S.n_actions = S.kind == SSD_ENV_CLEANUP ? 9 : 8;
    S.env_id_base = cfg->env_id_base; S.seed_lo = (uint32_t)cfg->seed; S.seed_hi = (uint32_t)(cfg->seed >> 32);
    S.magic_W = magic(S.W); S.magic_V = magic(S.V); S.magic_VV = magic(S.VV); S.magic_3VV = magic(3 * S.VV); S.magic_HW = magic(S.HW);
    S.thr_dep = cfg->threshold_depletion; S.thr_res = cfg->threshold_restoration;
    S.p_waste = cfg->waste_spawn_prob; S.p_apple = cfg->apple_respawn_prob;
    for (int i = 0; i < 4; ++i) { S.harvest_p[i] = cfg->harvest_spawn_prob[i]; S.harvest_thr[i] = draw_threshold(S.harvest_p[i]); }
    if ((long)S.n * 3 * S.VV >= 65536) { delete E; return fail(SSD_ERR_INVALID, "n_agents * 3 * V * V must stay below 65536"); }
    // the slice k_env actually reserves per wave (launch_env), and the class-code gather's write range inside its planes (any team
    // size can take the run-time instantiation: TAPE mode, render mode)
    if ((long)lds_per_wave(S) * kWavesPerBlock > 160 * 1024) { delete E; return fail(SSD_ERR_INVALID, "k_env's LDS slices exceed the 160 KiB of a workgroup"); }
    if (code_gather_end(S, kCodeGroupMax) > lds_planes_bytes(S)) { delete E; return fail(SSD_ERR_INVALID, "class-code gather overruns its LDS planes"); }

    // Row-major scan of the layout (map_env.py:143-148, cleanup.py:77-90, harvest.py:31-35).
    std::vector<int> spawn;
    for (int i = 0; i < S.HW; ++i) {
        const char ch = cfg->ascii_map[i];
        uint8_t code = C_EMPTY;
        bool overflow = false;
        if (ch == '@') code = C_WALL;
        else if (ch == 'P') spawn.push_back(i);
        else if (S.kind == SSD_ENV_CLEANUP) {
            if (ch == 'B') { if (S.n_apple < SSD_MAX_SITES) S.apple[S.n_apple++] = (uint16_t)i; else overflow = true; }
            else if (ch == 'H') { code = C_WASTE; if (S.n_waste < SSD_MAX_SITES) S.waste[S.n_waste++] = (uint16_t)i; else overflow = true; }
            else if (ch == 'R') code = C_RIVER;
            else if (ch == 'S') code = C_STREAM;
        } else if (ch == 'A') { code = C_APPLE; if (S.n_apple < SSD_MAX_SITES) S.apple[S.n_apple++] = (uint16_t)i; else overflow = true; }
        if (overflow) { delete E; return fail(SSD_ERR_INVALID, "too many apple / waste sites (max 256)"); }
        S.reset_grid[i] = code;
    }
    // compute_probabilities (cleanup.py:189-204) for every possible waste count, reference operation order, plain fp64
    for (int current = 0; current <= SSD_MAX_SITES; ++current) {
        volatile double wd = 0, pa = 0, pw = 0;
        const int potential = S.n_waste;
        if (potential > 0) {
            const int free_area = potential - current;
            volatile double q = (double)free_area / (double)potential;
            wd = 1 - q;
        }
        if (!(wd >= S.thr_dep)) {
            pw = S.p_waste;
            if (wd <= S.thr_res) pa = S.p_apple;
            else {
                volatile double num = wd - S.thr_res, den = S.thr_dep - S.thr_res;
                volatile double frac = num / den;
                volatile double one_minus = 1 - frac;
                pa = one_minus * S.p_apple;
            }
        }
        S.tab_p[current][0] = pa; S.tab_p[current][1] = pw;
        const double pa_ = pa, pw_ = pw;
        S.tab_thr[current][0] = draw_threshold(pa_); S.tab_thr[current][1] = draw_threshold(pw_);
        S.tab_thr[current][2] = (pa_ > 0 ? 1u : 0u) | (!(std::fabs(pw_) <= 1e-8) ? 2u : 0u);
        S.tab_thr[current][3] = 0;
    }
    for (int a = 0; a <= SSD_MAX_CELLS; ++a) S.tab_den[a] = (float)((double)a / (double)S.HW);
    for (int l = 0; l < 64; ++l)
        for (int ch = 0; ch < 4; ++ch) {
            S.site_t[l][ch] = ch * 64 + l < S.n_apple ? S.apple[ch * 64 + l] : (uint16_t)0;
            S.site_t[l][4 + ch] = ch * 64 + l < S.n_waste ? S.waste[ch * 64 + l] : (uint16_t)0;
        }
    E->n_spawn = (int)spawn.size();
    S.random_spawn = cfg->random_spawn_point ? 1 : 0; S.n_spawn = (int)spawn.size();
    S.spawn_len = (S.kind == SSD_ENV_CLEANUP ? 2 : 1) * S.n_spawn;   // Cleanup's constructor appends every point again (cleanup.py:79-80)
    if (S.random_spawn && spawn.size() > SSD_MAX_SPAWN) { delete E; return fail(SSD_ERR_UNSUPPORTED, "random_spawn_point supports at most SSD_MAX_SPAWN spawn points"); }
    for (size_t i = 0; i < spawn.size() && i < SSD_MAX_SPAWN; ++i) S.spawn_all[i] = (uint16_t)spawn[i];
    if ((int)spawn.size() < S.n) { delete E; return fail(SSD_ERR_INVALID, "There are not enough spawn points! Check your map?"); }
    // spawn_point() returns the LAST free spawn point (map_env.py:779-784): agent a gets the a-th from the end.
    for (int a = 0; a < S.n; ++a) S.spawn_cell[a] = (uint16_t)spawn[spawn.size() - 1 - a];
    // agents must never stand on the border (the kernels index t = P +- W, P +- 1 without a bounds test on rows)
    for (int a = 0; a < S.n; ++a) {
        const int r = S.spawn_cell[a] / S.W, c = S.spawn_cell[a] % S.W;
        if (r == 0 || c == 0 || r == S.H - 1 || c == S.W - 1) { delete E; return fail(SSD_ERR_INVALID, "spawn point on the map border"); }
    }
    for (int i = 0; i < S.HW; ++i) {
        const int r = i / S.W, c = i % S.W;
        if ((r == 0 || c == 0 || r == S.H - 1 || c == S.W - 1) && S.reset_grid[i] != C_WALL) {
            delete E; return fail(SSD_ERR_INVALID, "the map border must be wall ('@')");
        }
    }
    // Full-colour LUT (map_env.py:33-62 DEFAULT_COLOURS; cleanup.py:14-17 CLEANUP_COLORS), rows: cell codes 0..5, then 5 + agent char.
    static const uint8_t agent_rgb[10][3] = {{0, 0, 0}, {159, 67, 255}, {2, 81, 154}, {204, 0, 204}, {216, 30, 54},
                                             {254, 151, 0}, {205, 155, 155}, {99, 99, 255}, {250, 204, 255}, {238, 223, 16}};
    uint8_t (*lut)[3] = (uint8_t (*)[3])S.lut;
    lut[C_WALL][0] = lut[C_WALL][1] = lut[C_WALL][2] = 180;
    lut[C_APPLE][1] = 255;
    if (S.kind == SSD_ENV_CLEANUP) {
        lut[C_WASTE][0] = 99; lut[C_WASTE][1] = 156; lut[C_WASTE][2] = 194;
        lut[C_RIVER][0] = lut[C_STREAM][0] = 113; lut[C_RIVER][1] = lut[C_STREAM][1] = 75; lut[C_RIVER][2] = lut[C_STREAM][2] = 24;
    }
    for (int ch = 1; ch <= 9; ++ch) std::memcpy(lut[5 + ch], agent_rgb[ch], 3);
    // the render table (ssd_render): the same 15 rows, then 'F' (yellow, DEFAULT_COLOURS) and 'C' (cyan, CLEANUP_COLORS; Cleanup only)
    std::memcpy(E->host_lut, S.lut, 15 * 3);
    E->host_lut[15 * 3] = 255; E->host_lut[15 * 3 + 1] = 255; E->host_lut[15 * 3 + 2] = 0;
    if (S.kind == SSD_ENV_CLEANUP) { E->host_lut[16 * 3] = 100; E->host_lut[16 * 3 + 1] = 255; E->host_lut[16 * 3 + 2] = 255; }

    // ---- device side ----
    int prev = 0;
    E->device = cfg->device;
    hipError_t e = hipGetDevice(&prev);
    if (e == hipSuccess) e = hipSetDevice(cfg->device);
    const size_t N = (size_t)S.N, n = (size_t)S.n;
    if (e == hipSuccess) e = hipMalloc((void**)&E->dspec, sizeof(DevSpec));
    if (e == hipSuccess) e = hipMalloc((void**)&E->st.grid, N * S.GS);
    if (e == hipSuccess) e = hipMalloc((void**)&E->st.agents, N * n * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&E->st.hdr, N * sizeof(ssd::EnvHdr));
    if (e == hipSuccess) e = hipMalloc((void**)&E->st.err, 4);
    if (e == hipSuccess) e = hipMemcpy(E->dspec, &S, sizeof(DevSpec), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(E->st.grid, 0, N * S.GS);
    if (e == hipSuccess) e = hipMemset(E->st.agents, 0, N * n * 8);
    if (e == hipSuccess) {      // counts unknown (recount at the first step), everything else 0
        std::vector<ssd::EnvHdr> hz(N);
        memset(hz.data(), 0, N * sizeof(ssd::EnvHdr));
        for (size_t i = 0; i < N; ++i) hz[i].counts = 0xFFFFFFFFu;
        e = hipMemcpy(E->st.hdr, hz.data(), N * sizeof(ssd::EnvHdr), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipMemset(E->st.err, 0, 4);
    if (e == hipSuccess && !numeric_err_word()) e = hipErrorOutOfMemory;      // exists before anything captures a graph
    if (e == hipSuccess && !bmm_scratch(nullptr)) e = hipErrorOutOfMemory;           // (the affine layers' backward scratch: same reason)
    if (e == hipSuccess) {
        // a fresh handle holds the reset image with agents on their spawn cells (the reference constructor
        // also builds agents before the first reset, map_env.py:149)
        std::vector<uint8_t> g((size_t)S.GS, 0);
        std::memcpy(g.data(), S.reset_grid, (size_t)S.HW);
        std::vector<uint32_t> rec(n);
        for (size_t a = 0; a < n; ++a) {
            const uint32_t r = S.spawn_cell[a] / S.W, c = S.spawn_cell[a] % S.W;
            rec[a] = r | (c << 8) | ((uint32_t)(S.spawn_rotation < 0 ? 0 : S.spawn_rotation) << 16);
        }
        std::vector<uint8_t> gall(N * S.GS);
        std::vector<uint32_t> rall(N * n * 2, 0u);      // {arec, episode reward = 0}
        for (size_t i = 0; i < N; ++i) {
            std::memcpy(&gall[i * S.GS], g.data(), (size_t)S.GS);
            for (size_t a = 0; a < n; ++a) rall[(i * n + a) * 2] = rec[a];
        }
        e = hipMemcpy(E->st.grid, gall.data(), gall.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(E->st.agents, rall.data(), rall.size() * 4, hipMemcpyHostToDevice);
    }
    (void)hipSetDevice(prev);
    if (e != hipSuccess) {
        fail(SSD_ERR_DEVICE, "device setup failed: %s", hipGetErrorString(e));
        ssd_destroy(E);
        return SSD_ERR_DEVICE;
    }
    *out = E;
    return SSD_OK;
}

int ssd_destroy(ssd_env* E) {
    if (!E) return SSD_OK;
    (void)hipFree(E->beam_rec); (void)hipFree(E->render_lut);
    (void)hipFree(E->dspec); (void)hipFree(E->st.grid); (void)hipFree(E->st.agents); (void)hipFree(E->st.hdr); (void)hipFree(E->st.err);
    delete E;
    return SSD_OK;
}

int ssd_get_info(const ssd_env* E, ssd_info* o) {
    if (!E || !o) return fail(SSD_ERR_INVALID, "null argument");
    o->n_actions = E->hs.n_actions; o->n_apple_sites = E->hs.n_apple; o->n_waste_sites = E->hs.n_waste;
    o->n_spawn_points = E->n_spawn; o->max_uniforms = E->hs.n_apple + E->hs.n_waste; o->obs_edge = E->hs.V;
    return SSD_OK;
}

static int make_tape(const ssd_env* E, const ssd_tape* t, DevTape* d) {
    std::memset(d, 0, sizeof *d);
    if (E->hs.rng_mode == SSD_RNG_TAPE) {
        if (!t || !t->uniforms || !t->move_order) return fail(SSD_ERR_INVALID, "TAPE mode needs tape.uniforms and tape.move_order");
        if (E->hs.kind == SSD_ENV_CLEANUP && E->hs.n_waste > 0 && !t->waste_order) return fail(SSD_ERR_INVALID, "TAPE mode needs tape.waste_order for Cleanup");
        if (E->hs.spawn_rotation < 0 && !t->spawn_rot) return fail(SSD_ERR_INVALID, "TAPE mode with random rotation needs tape.spawn_rot");
        if (t->uniforms_stride < 1) return fail(SSD_ERR_INVALID, "tape.uniforms_stride");
    }
    if (t) { d->move_order = t->move_order; d->uniforms = t->uniforms; d->ustride = t->uniforms_stride; d->waste_order = t->waste_order; d->spawn_rot = t->spawn_rot;
             d->spawn_order = t->spawn_order; }
    return SSD_OK;
}
static DevStepOut make_so(const ssd_step_out* o) {
    DevStepOut d; std::memset(&d, 0, sizeof d);
    if (o) { d.reward = o->reward; d.clean_num = o->clean_num; d.apple_den = o->apple_den; d.terminated = o->terminated;
             d.collective = o->collective_return; d.equality = o->equality; d.n_draws = o->n_draws; }
    return d;
}
static int make_oo(const ssd_env* E, const ssd_obs_out* o, DevObsOut* d) {
    std::memset(d, 0, sizeof *d);
    if (!o) return fail(SSD_ERR_INVALID, "null ssd_obs_out");
    if (o->obs) {
        if (o->obs_format < SSD_OBS_F32 || o->obs_format > SSD_OBS_CODE) return fail(SSD_ERR_INVALID, "obs_format");
        if (o->obs_format == SSD_OBS_CODE && E->hs.obs_color != SSD_COLOR_SIMPLIFIED) return fail(SSD_ERR_INVALID, "SSD_OBS_CODE needs simplified colours");
        if (((uintptr_t)o->obs & 15) != 0) return fail(SSD_ERR_INVALID, "obs must be 16-byte aligned");
    }
    if (o->state && ((uintptr_t)o->state & 15) != 0) return fail(SSD_ERR_INVALID, "state must be 16-byte aligned");
    if (o->obs_env_stride < 0 || o->obs_slot_stride < 0 || (!o->obs_env_stride && o->obs_slot_stride))
        return fail(SSD_ERR_INVALID, "obs_env_stride / obs_slot_stride");
    if (o->obs_t_slots < 0) return fail(SSD_ERR_INVALID, "obs_t_slots");
    if (o->obs_code) {
        if (!o->obs || o->obs_format == SSD_OBS_CODE) return fail(SSD_ERR_INVALID, "obs_code accompanies a f32 / bf16 / u8 obs output");
        if (E->hs.obs_color != SSD_COLOR_SIMPLIFIED) return fail(SSD_ERR_INVALID, "obs_code needs simplified colours");
        if (((uintptr_t)o->obs_code & 15) != 0) return fail(SSD_ERR_INVALID, "obs_code must be 16-byte aligned");
    }
    d->obs = o->obs; d->fmt = o->obs_format; d->state = o->state; d->pos = o->pos; d->orient = o->orient;
    d->env_stride = (long)o->obs_env_stride; d->slot_stride = (long)o->obs_slot_stride;
    d->t_slots = o->obs_t_slots; d->code = o->obs_code; d->code_agent_stride = SSD_CODE_AGENT_STRIDE(E->hs.V);
    d->stamps = E->st.stamps;
    return SSD_OK;
}
}   // extern "C" (reopened below): the numeric-status word is a C++ helper of namespace ssd
namespace ssd {
int32_t* numeric_err_word() {
    static int32_t* word[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    if (!word[dev]) {
        int32_t* w = nullptr;
        if (hipMalloc((void**)&w, 64) != hipSuccess || hipMemset(w, 0, 64) != hipSuccess) return nullptr;
        word[dev] = w;
    }
    return word[dev];
}
}  // namespace ssd
extern "C" {

static int launched(void) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SSD_ERR_DEVICE, "kernel launch failed: %s", hipGetErrorString(e));
    return SSD_OK;
}

int ssd_reset(ssd_env* E, const uint8_t* env_mask, const ssd_tape* tape, ssd_step_out* out, void* stream) {
    if (!E) return fail(SSD_ERR_INVALID, "null env");
    DevTape t; if (int rc = make_tape(E, tape, &t)) return rc;
    if (E->hs.rng_mode == SSD_RNG_TAPE && E->hs.random_spawn && !t.spawn_order) return fail(SSD_ERR_INVALID, "TAPE mode with random_spawn_point needs tape.spawn_order");
    DevObsOut oo; std::memset(&oo, 0, sizeof oo);
    launch_env(MODE_RESET, E->dspec, E->hs, E->st, nullptr, env_mask, t, make_so(out), oo, (hipStream_t)stream);
    if (E->beam_rec) launch_beam_clear(E->beam_rec, env_mask, E->hs.N, E->hs.n, (hipStream_t)stream);
    return launched();
}

int ssd_step(ssd_env* E, const int32_t* actions, const ssd_tape* tape, ssd_step_out* out, void* stream) {
    if (!E || !actions) return fail(SSD_ERR_INVALID, "null argument");
    DevTape t; if (int rc = make_tape(E, tape, &t)) return rc;
    DevObsOut oo; std::memset(&oo, 0, sizeof oo);
    launch_env(MODE_STEP, E->dspec, E->hs, E->st, actions, nullptr, t, make_so(out), oo, (hipStream_t)stream, E->beam_rec);
    return launched();
}

int ssd_observe(ssd_env* E, ssd_obs_out* out, void* stream) {
    if (!E) return fail(SSD_ERR_INVALID, "null env");
    DevObsOut oo; if (int rc = make_oo(E, out, &oo)) return rc;
    DevTape t; std::memset(&t, 0, sizeof t);
    launch_env(MODE_OBS, E->dspec, E->hs, E->st, nullptr, nullptr, t, make_so(nullptr), oo, (hipStream_t)stream);
    return launched();
}

int ssd_step_observe(ssd_env* E, const int32_t* actions, const ssd_tape* tape, ssd_step_out* out, ssd_obs_out* obs, void* stream) {
    if (!E || !actions) return fail(SSD_ERR_INVALID, "null argument");
    DevTape t; if (int rc = make_tape(E, tape, &t)) return rc;
    DevObsOut oo; if (int rc = make_oo(E, obs, &oo)) return rc;
    launch_env(MODE_STEP_OBS, E->dspec, E->hs, E->st, actions, nullptr, t, make_so(out), oo, (hipStream_t)stream, E->beam_rec);
    return launched();
}

int ssd_set_render(ssd_env* E, int32_t on) {
    if (!E) return fail(SSD_ERR_INVALID, "null env");
    if ((on != 0) == (E->beam_rec != nullptr)) return SSD_OK;
    int prev = 0;
    HIP_TRY(hipGetDevice(&prev));
    HIP_TRY(hipSetDevice(E->device));
    hipError_t e = hipSuccess;
    if (on) {
        const size_t bytes = (size_t)E->hs.N * E->hs.n * sizeof(uint32_t);
        e = hipMalloc((void**)&E->beam_rec, bytes);
        if (e == hipSuccess) e = hipMalloc((void**)&E->render_lut, sizeof E->host_lut);
        if (e == hipSuccess) e = hipMemcpy(E->render_lut, E->host_lut, sizeof E->host_lut, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(E->beam_rec, 0, bytes);      // no beams until the first step
        if (e != hipSuccess) { (void)hipFree(E->beam_rec); (void)hipFree(E->render_lut); E->beam_rec = nullptr; E->render_lut = nullptr; }
    } else {
        e = hipDeviceSynchronize();                                    // launches in flight may still write the record
        (void)hipFree(E->beam_rec); (void)hipFree(E->render_lut);
        E->beam_rec = nullptr; E->render_lut = nullptr;
    }
    (void)hipSetDevice(prev);
    if (e != hipSuccess) return fail(SSD_ERR_DEVICE, "ssd_set_render: %s", hipGetErrorString(e));
    return SSD_OK;
}

int ssd_render(ssd_env* E, const int32_t* env_ids, int32_t n_sel, uint8_t* frames, const int32_t* slot, int64_t slot_stride, void* stream) {
    if (!E || !env_ids || !frames) return fail(SSD_ERR_INVALID, "null argument");
    if (!E->beam_rec) return fail(SSD_ERR_INVALID, "ssd_render needs render mode (ssd_set_render)");
    if (n_sel < 1) return fail(SSD_ERR_INVALID, "n_sel must be >= 1");
    if (slot_stride < 0) return fail(SSD_ERR_INVALID, "slot_stride must be >= 0");
    launch_render(E->dspec, E->hs, E->st, E->beam_rec, E->render_lut, env_ids, n_sel, frames, slot, (long long)slot_stride, (hipStream_t)stream);
    return launched();
}

#ifdef SSD_STAMPS
// diagnostic build only: device buffer [n_env, 32] of u64 receiving the phase stamps
int ssd_debug_set_stamps(ssd_env* E, unsigned long long* buf) { E->st.stamps = buf; return SSD_OK; }
int ssd_debug_set_policy_stamps(unsigned long long* buf) { ssd::set_policy_stamps(buf); return SSD_OK; }
#endif

int ssd_poll_error(ssd_env* E, int32_t* bits) {
    if (!E || !bits) return fail(SSD_ERR_INVALID, "null argument");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(bits, E->st.err, 4, hipMemcpyDeviceToHost));
    if (*bits) HIP_TRY(hipMemset(E->st.err, 0, 4));
    int32_t num = 0;                                                   // + the device's numeric status (SSD_ERRBIT_F16_RANGE)
    if (int rc = ssd_numeric_status(&num)) return rc;
    *bits |= num;
    return SSD_OK;
}

int ssd_numeric_status(int32_t* bits) {
    if (!bits) return fail(SSD_ERR_INVALID, "null argument");
    int32_t* w = numeric_err_word();
    if (!w) return fail(SSD_ERR_DEVICE, "numeric status word: allocation failed");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(bits, w, 4, hipMemcpyDeviceToHost));
    if (*bits) HIP_TRY(hipMemset(w, 0, 4));
    return SSD_OK;
}

int ssd_export_state(ssd_env* E, ssd_state* dst, void* stream) {
    if (!E || !dst) return fail(SSD_ERR_INVALID, "null argument");
    launch_export(E->dspec, E->hs, E->st, *dst, (hipStream_t)stream);
    return launched();
}

int ssd_import_state(ssd_env* E, const ssd_state* src, void* stream) {
    if (!E || !src) return fail(SSD_ERR_INVALID, "null argument");
    launch_import(E->dspec, E->hs, E->st, *src, (hipStream_t)stream);
    return launched();
}

// ssd_build_inputs / _flags: the kernels take the row count batch * n_agents as an `int` (the element index and the grid are 64-bit):
// any team size and action count whose row count and widest row (every block of the flag word present) stay below 2^31 is computed,
// anything larger refused.  ssd_unroll_other / ssd_td_sim_loss form the thread index in `int` as well: SSD_ROWS32_MAX
static bool build_inputs_fits(int64_t batch, int64_t n, int64_t A, int64_t out_offset) {
    return batch * n <= INT32_MAX && out_offset >= 0 && out_offset + n * A + A + 2 * n + 4 <= INT32_MAX;
}

int ssd_build_inputs(int32_t batch, int32_t n_agents, int32_t n_actions, int32_t t0, const int64_t* last_actions,
                     const float* last_reward, const int64_t* last_actions_inc, const float* pos, float pos_scale,
                     float* out, int32_t out_stride, int32_t out_offset, void* stream) {
    if (batch < 1 || n_agents < 1 || n_actions < 1 || !out || !pos) return fail(SSD_ERR_INVALID, "bad argument");
    if (!build_inputs_fits(batch, n_agents, n_actions, out_offset)) return fail(SSD_ERR_INVALID, "ssd_build_inputs: batch * n_agents and the row width must fit 32 bits, out_offset >= 0");
    if (!(t0 & 1) && (!last_actions || !last_reward || !last_actions_inc)) return fail(SSD_ERR_INVALID, "t > 0 needs the t-1 tensors");
    if (out_stride < out_offset + n_actions + n_agents + 4) return fail(SSD_ERR_INVALID, "out_stride too small");
    launch_build_inputs(batch, n_agents, n_actions, t0, last_actions, last_reward, last_actions_inc, pos, pos_scale, out,
                        out_stride, out_offset, (hipStream_t)stream);
    return launched();
}

int ssd_unroll_other(const int64_t* actions, const float* pos, const float* orient, const float* reward, const float* clean_num, const float* apple_den,
                     float pos_scale, int32_t batch, int32_t T, int32_t n_agents, int32_t n_actions, float* other, float* act_tm, void* stream) {
    if (!actions || !pos || !orient || !reward || !clean_num || !apple_den || !other || !act_tm || batch < 1 || T < 1 || n_agents < 1 || n_actions < 1 ||
        !(pos_scale > 0.f)) return fail(SSD_ERR_INVALID, "bad argument");
    if ((int64_t)batch * T * n_agents > SSD_ROWS32_MAX || n_actions > INT32_MAX - 7) return fail(SSD_ERR_INVALID, "ssd_unroll_other: batch * T * n_agents over SSD_ROWS32_MAX");
    launch_unroll_other(actions, pos, orient, reward, clean_num, apple_den, pos_scale, batch, T, n_agents, n_actions, other, act_tm, (hipStream_t)stream);
    return launched();
}

int ssd_incentive_transfer(int32_t batch, int32_t T, int32_t n_agents, const int64_t* actions_inc, const float* rewards,
                           float effect_ratio, float cost_ratio, float incentive, float seq_len, float* give,
                           float* recv_pos, float* recv_neg, float* recv_zero, float* rewards_for_env,
                           float* rewards_for_inc, void* stream) {
    if (batch < 1 || T < 2 || n_agents < 1 || !actions_inc || !rewards || !give || !recv_pos || !recv_neg || !recv_zero ||
        !rewards_for_env || !rewards_for_inc)
        return fail(SSD_ERR_INVALID, "bad argument");
    launch_incentive_transfer(batch, T, n_agents, actions_inc, rewards, effect_ratio, cost_ratio, incentive, seq_len, give,
                              recv_pos, recv_neg, recv_zero, rewards_for_env, rewards_for_inc, (hipStream_t)stream);
    return launched();
}

int ssd_column_sums(const float* x, float* out, int32_t groups, int32_t rows, int32_t cols, float* workspace, void* stream) {
    if (!x || !out || groups < 1 || rows < 1 || cols < 1 || groups > 65535 || (rows + SSD_COLSUM_CHUNK - 1) / SSD_COLSUM_CHUNK > 65535)
        return fail(SSD_ERR_INVALID, "bad argument");
    launch_column_sums(x, out, groups, rows, cols, workspace, (hipStream_t)stream);
    return launched();
}

int ssd_build_inputs_width(int32_t n_agents, int32_t n_actions, uint32_t input_flags) {
    if (n_agents < 1 || n_actions < 1 || ((input_flags & ~SSD_INPUT_EXPLICIT) & ~127u)) return -1;
    return build_inputs_layout(n_agents, n_actions, input_flags).width;
}

int ssd_build_inputs_flags(int32_t batch, int32_t n_agents, int32_t n_actions, int32_t t0, uint32_t input_flags, const int64_t* last_actions,
                           const float* last_reward, const int64_t* last_actions_inc, const float* pos, float pos_scale, float* out,
                           int32_t out_stride, int32_t out_offset, void* stream) {
    if (batch < 1 || n_agents < 1 || n_actions < 1 || !out || !pos) return fail(SSD_ERR_INVALID, "bad argument");
    if (!build_inputs_fits(batch, n_agents, n_actions, out_offset)) return fail(SSD_ERR_INVALID, "ssd_build_inputs_flags: batch * n_agents and the row width must fit 32 bits, out_offset >= 0");
    if ((input_flags & ~SSD_INPUT_EXPLICIT) & ~127u) return fail(SSD_ERR_UNSUPPORTED, "ssd_build_inputs_flags: unknown input_flags bit");
    if (!(t0 & 1) && (!last_actions || !last_reward || !last_actions_inc)) return fail(SSD_ERR_INVALID, "t > 0 needs the t-1 tensors");
    if (out_stride < out_offset + build_inputs_layout(n_agents, n_actions, input_flags).width) return fail(SSD_ERR_INVALID, "out_stride too small");
    launch_build_inputs_flags(batch, n_agents, n_actions, t0, input_flags, last_actions, last_reward, last_actions_inc, pos, pos_scale, out,
                              out_stride, out_offset, (hipStream_t)stream);
    return launched();
}

int ssd_clip_adam_step(const ssd_clip_adam_args* a, void* stream) {
    if (!a || !a->flat_grad || !a->jobs || !a->partials || a->total < 1 || a->n_jobs < 1 || a->n_jobs > SSD_ADAM_MAX_JOBS)
        return fail(SSD_ERR_INVALID, "ssd_clip_adam_step: bad argument");
    if (a->total > (int64_t)INT32_MAX) return fail(SSD_ERR_INVALID, "ssd_clip_adam_step: total");
    if (!(a->beta1 >= 0.f && a->beta1 < 1.f) || !(a->beta2 >= 0.f && a->beta2 < 1.f) || !(a->eps > 0.f) || !(a->clip > 0.f))
        return fail(SSD_ERR_INVALID, "ssd_clip_adam_step: betas / eps / clip");
    // the Polyak target update behind the Adam launch (all zero / NULL: none)
    if (a->n_polyak < 0 || a->n_polyak > SSD_POLYAK_MAX_JOBS) return fail(SSD_ERR_INVALID, "ssd_clip_adam_step: n_polyak outside 0 .. SSD_POLYAK_MAX_JOBS");
    if (a->n_polyak > 0 && !a->polyak_jobs) return fail(SSD_ERR_INVALID, "ssd_clip_adam_step: n_polyak > 0 without polyak_jobs");
    if (!(a->target_tau >= 0.f && a->target_tau <= 1.f)) return fail(SSD_ERR_INVALID, "ssd_clip_adam_step: target_tau outside [0, 1]");
    if (a->n_polyak > 0 && a->target_tau == 0.f) return fail(SSD_ERR_INVALID, "ssd_clip_adam_step: n_polyak > 0 with target_tau 0 (an update that moves nothing)");
    launch_clip_adam(a, (hipStream_t)stream);
    return launched();
}

int ssd_dueling_q_fwd(const float* a, const float* v, float* q, int32_t n, int32_t T, int32_t B, int32_t inner, int32_t K, void* stream) {
    if (!a || !v || !q || n < 1 || T < 1 || B < 1 || inner < 1 || K < 1 || K > 16) return fail(SSD_ERR_INVALID, "ssd_dueling_q_fwd: bad argument");
    launch_dueling_q(a, v, q, nullptr, nullptr, nullptr, n, T, B, inner, K, (hipStream_t)stream);
    return launched();
}
int ssd_dueling_q_bwd(const float* dq, float* da, float* dv, int32_t n, int32_t T, int32_t B, int32_t inner, int32_t K, void* stream) {
    if (!dq || !da || !dv || n < 1 || T < 1 || B < 1 || inner < 1 || K < 1 || K > 16) return fail(SSD_ERR_INVALID, "ssd_dueling_q_bwd: bad argument");
    launch_dueling_q(nullptr, nullptr, nullptr, dq, da, dv, n, T, B, inner, K, (hipStream_t)stream);
    return launched();
}

int ssd_gather_rows(const ssd_row_gather* fields, int32_t count, const int64_t* ids, int32_t n_ids, void* stream) {
    if (!fields || count < 1 || count > SSD_COPY_BLOCKS_MAX || !ids || n_ids < 1 || n_ids > 65535) return fail(SSD_ERR_INVALID, "ssd_gather_rows: bad argument");
    for (int i = 0; i < count; ++i)
        if (!fields[i].src || !fields[i].dst || fields[i].row_bytes < 1) return fail(SSD_ERR_INVALID, "ssd_gather_rows: bad field");
    launch_gather_rows(fields, count, ids, n_ids, (hipStream_t)stream);
    return launched();
}

int ssd_sample_ids(uint64_t seed, uint32_t call, int32_t population, int32_t count, int64_t* ids, void* stream) {
    if (!ids || count < 1 || count > SSD_SAMPLE_IDS_MAX || population < count) return fail(SSD_ERR_INVALID, "ssd_sample_ids: 1 <= count <= min(population, SSD_SAMPLE_IDS_MAX)");
    launch_sample_draw(seed, call, population, count, 1, ids, nullptr, (hipStream_t)stream);
    return launched();
}

int ssd_copy_blocks(const ssd_block_copy* blocks, int32_t count, void* stream) {
    if (!blocks || count < 1 || count > SSD_COPY_BLOCKS_MAX) return fail(SSD_ERR_INVALID, "ssd_copy_blocks: 1..SSD_COPY_BLOCKS_MAX blocks");
    for (int i = 0; i < count; ++i) {
        const ssd_block_copy& b = blocks[i];
        if (!b.src || !b.dst || b.rows < 1 || b.cols < 1 || b.src_stride < b.cols || b.dst_stride < b.cols ||
            (int64_t)b.rows * b.cols > SSD_COPY_BLOCK_ELEMS_MAX)
            return fail(SSD_ERR_INVALID, "ssd_copy_blocks: bad block");
    }
    launch_copy_blocks(blocks, count, (hipStream_t)stream);
    return launched();
}

int ssd_fill_blocks(const ssd_block_fill* blocks, int32_t count, void* stream) {
    if (!blocks || count < 1 || count > SSD_FILL_BLOCKS_MAX) return fail(SSD_ERR_INVALID, "ssd_fill_blocks: 1..SSD_FILL_BLOCKS_MAX blocks");
    for (int i = 0; i < count; ++i)
        if (!blocks[i].dst || blocks[i].bytes < 4 || (blocks[i].bytes & 3) || ((uintptr_t)blocks[i].dst & 3)) return fail(SSD_ERR_INVALID, "ssd_fill_blocks: a block is a 4-byte aligned multiple of 4 bytes");
    launch_fill_blocks(blocks, count, (hipStream_t)stream);
    return launched();
}
int ssd_runner_stats(const float* collective_return, const float* equality, const float* episode_return, int32_t n_env, int32_t n_returns,
                     double* acc, void* stream) {
    if (!collective_return || !equality || !episode_return || !acc || n_env < 1 || n_returns < 1) return fail(SSD_ERR_INVALID, "bad argument");
    launch_runner_stats(collective_return, equality, episode_return, n_env, n_returns, acc, (hipStream_t)stream);
    return launched();
}
int ssd_sample_windows(uint64_t seed, uint32_t call, int32_t population, int32_t count, int32_t n_starts, int64_t* ids, int64_t* t0, void* stream) {
    if (!ids || !t0) return fail(SSD_ERR_INVALID, "ssd_sample_windows: null pointer");
    if (count < 1 || count > SSD_SAMPLE_IDS_MAX || population < count) return fail(SSD_ERR_INVALID, "ssd_sample_windows: 1 <= count <= min(population, SSD_SAMPLE_IDS_MAX)");
    if (n_starts < 1) return fail(SSD_ERR_INVALID, "ssd_sample_windows: n_starts >= 1");
    launch_sample_draw(seed, call, population, count, n_starts, ids, t0, (hipStream_t)stream);
    return launched();
}

int ssd_gather_windows(const ssd_window_field* fields, int32_t count, const int64_t* ids, const int64_t* t0, int32_t n_ids, int32_t src_slots,
                       int32_t win_slots, int32_t burn_in, void* stream) {
    if (!fields || !ids || !t0) return fail(SSD_ERR_INVALID, "ssd_gather_windows: null pointer");
    if (count < 1 || count > SSD_COPY_BLOCKS_MAX) return fail(SSD_ERR_INVALID, "ssd_gather_windows: 1..SSD_COPY_BLOCKS_MAX fields");
    if (n_ids < 1 || n_ids > 65535) return fail(SSD_ERR_INVALID, "ssd_gather_windows: n_ids outside 1 .. 65535");
    if (win_slots < 2 || win_slots > src_slots) return fail(SSD_ERR_INVALID, "ssd_gather_windows: win_slots outside 2 .. src_slots");
    if (burn_in < 0 || burn_in > win_slots - 2) return fail(SSD_ERR_INVALID, "ssd_gather_windows: burn_in outside 0 .. win_slots - 2");
    int n_filled = 0;
    for (int i = 0; i < count; ++i) {
        const ssd_window_field& f = fields[i];
        if (!f.src || !f.dst || f.slot_bytes < 1) return fail(SSD_ERR_INVALID, "ssd_gather_windows: bad field (null pointer or slot_bytes < 1)");
        // the grid is one workgroup per 8 KiB of destination: 64 GiB per field keeps the sum over 32 fields inside a 32-bit grid
        if (f.slot_bytes > (int64_t)(1ll << 36) / ((int64_t)n_ids * win_slots)) return fail(SSD_ERR_INVALID, "ssd_gather_windows: a field's destination is over 64 GiB");
        if (f.filled) {
            ++n_filled;
            if (n_filled > 1 || f.slot_bytes != 8 || (reinterpret_cast<uintptr_t>(f.src) & 7) || (reinterpret_cast<uintptr_t>(f.dst) & 7))
                return fail(SSD_ERR_INVALID, "ssd_gather_windows: at most one filled field, of 8-byte slots at 8-byte aligned pointers");
        }
    }
    launch_gather_windows(fields, count, ids, t0, n_ids, src_slots, win_slots, burn_in, (hipStream_t)stream);
    return launched();
}

static bool unit_interval(float x) { return x >= 0.f && x <= 1.f; }          // (false for a NaN)
int ssd_priority_sample(const ssd_priority_sample_args* a, void* stream) {
    if (!a) return fail(SSD_ERR_INVALID, "ssd_priority_sample: null args");
    if (!a->table || !a->ids || !a->t0 || !a->weights || !a->log) return fail(SSD_ERR_INVALID, "ssd_priority_sample: null member pointer");
    if (a->population < 1 || a->population > SSD_PRIORITY_POP_MAX) return fail(SSD_ERR_INVALID, "ssd_priority_sample: population outside 1 .. SSD_PRIORITY_POP_MAX");
    if (a->count < 1 || a->count > SSD_SAMPLE_IDS_MAX) return fail(SSD_ERR_INVALID, "ssd_priority_sample: count outside 1 .. SSD_SAMPLE_IDS_MAX");
    if (a->n_starts < 1) return fail(SSD_ERR_INVALID, "ssd_priority_sample: n_starts >= 1");
    if (!unit_interval(a->beta)) return fail(SSD_ERR_INVALID, "ssd_priority_sample: beta outside [0, 1]");
    if (reinterpret_cast<uintptr_t>(a->table) & 3) return fail(SSD_ERR_INVALID, "ssd_priority_sample: table is not 4-byte aligned");
    if (a->n_segments < 0 || a->n_segments > SSD_PRIORITY_SEGMENTS_MAX) return fail(SSD_ERR_INVALID, "ssd_priority_sample: n_segments outside 0 .. SSD_PRIORITY_SEGMENTS_MAX");
    if (a->n_segments) {                                                     // a priority per window: population counts entries
        if (!a->entries) return fail(SSD_ERR_INVALID, "ssd_priority_sample: n_segments >= 1 with null entries");
        if (a->seg_stride < 1 || a->last_start < 0) return fail(SSD_ERR_INVALID, "ssd_priority_sample: seg_stride < 1 or last_start < 0");
        if ((int64_t)(a->n_segments - 1) * a->seg_stride < a->last_start) return fail(SSD_ERR_INVALID, "ssd_priority_sample: (n_segments - 1) * seg_stride does not reach last_start");
        if (a->population % a->n_segments) return fail(SSD_ERR_INVALID, "ssd_priority_sample: population is not a multiple of n_segments");
    }
    launch_priority_sample(a, (hipStream_t)stream);
    return launched();
}

int ssd_priority_update(const ssd_priority_update_args* a, void* stream) {
    if (!a) return fail(SSD_ERR_INVALID, "ssd_priority_update: null args");
    if (!a->partials || !a->ids || !a->weights || !a->dq_env || !a->dq_inc || !a->q_new || !a->table)
        return fail(SSD_ERR_INVALID, "ssd_priority_update: null member pointer");
    if (a->batch < 1 || a->batch > SSD_SAMPLE_IDS_MAX) return fail(SSD_ERR_INVALID, "ssd_priority_update: batch outside 1 .. SSD_SAMPLE_IDS_MAX");
    if (a->t_slots < 2 || a->n_agents < 1 || a->n_actions < 1) return fail(SSD_ERR_INVALID, "ssd_priority_update: t_slots >= 2, n_agents >= 1, n_actions >= 1");
    if (a->table_len < 1 || a->table_len > SSD_PRIORITY_POP_MAX) return fail(SSD_ERR_INVALID, "ssd_priority_update: table_len outside 1 .. SSD_PRIORITY_POP_MAX");
    if (!unit_interval(a->alpha) || !unit_interval(a->eta)) return fail(SSD_ERR_INVALID, "ssd_priority_update: alpha or eta outside [0, 1]");
    if (!(a->eps > 0.f)) return fail(SSD_ERR_INVALID, "ssd_priority_update: eps <= 0");
    if ((int64_t)a->batch * a->t_slots * a->n_agents > SSD_ROWS32_MAX) return fail(SSD_ERR_INVALID, "ssd_priority_update: batch * t_slots * n_agents over SSD_ROWS32_MAX");
    if ((reinterpret_cast<uintptr_t>(a->partials) & 15) || (reinterpret_cast<uintptr_t>(a->dq_env) & 3) || (reinterpret_cast<uintptr_t>(a->dq_inc) & 3))
        return fail(SSD_ERR_INVALID, "ssd_priority_update: partials not 16-byte aligned, or dq_env / dq_inc not 4-byte aligned");
    launch_priority_update(a, (hipStream_t)stream);
    return launched();
}

int ssd_rollout_priority(const ssd_rollout_priority_args* a, void* stream) {
    if (!a) return fail(SSD_ERR_INVALID, "ssd_rollout_priority: null args");
    if (!a->t_index || !a->q_env || !a->q_inc || !a->actions || !a->actions_inc || !a->reward || !a->terminated || !a->carry || !a->acc || !a->q_init)
        return fail(SSD_ERR_INVALID, "ssd_rollout_priority: null member pointer");
    if (a->n_env < 1 || a->n_env > (1 << 24) || a->t_slots < 2) return fail(SSD_ERR_INVALID, "ssd_rollout_priority: n_env outside 1 .. 2^24, or t_slots < 2");
    if (a->n_agents < 2 || a->n_agents > SSD_MAX_AGENTS) return fail(SSD_ERR_INVALID, "ssd_rollout_priority: n_agents outside 2 .. SSD_MAX_AGENTS");
    if (a->n_actions < 1 || a->n_actions > 16) return fail(SSD_ERR_INVALID, "ssd_rollout_priority: n_actions outside 1 .. 16");
    if (!(a->avail_bits & ((1u << a->n_actions) - 1u))) return fail(SSD_ERR_INVALID, "ssd_rollout_priority: avail_bits names no action below n_actions");
    if (!unit_interval(a->alpha) || !unit_interval(a->eta)) return fail(SSD_ERR_INVALID, "ssd_rollout_priority: alpha or eta outside [0, 1]");
    if (!(a->eps > 0.f)) return fail(SSD_ERR_INVALID, "ssd_rollout_priority: eps <= 0");
    if (!(a->seq_len > 0.f) || !(a->reward_scale > 0.f)) return fail(SSD_ERR_INVALID, "ssd_rollout_priority: seq_len or reward_scale <= 0");
    if (a->q_env_agent_stride < 0 || a->q_env_env_stride < 0 || a->q_inc_agent_stride < 0 || a->q_inc_env_stride < 0)
        return fail(SSD_ERR_INVALID, "ssd_rollout_priority: negative stride");
    if ((reinterpret_cast<uintptr_t>(a->q_env) | reinterpret_cast<uintptr_t>(a->q_inc) | reinterpret_cast<uintptr_t>(a->reward) | reinterpret_cast<uintptr_t>(a->carry)
         | reinterpret_cast<uintptr_t>(a->acc) | reinterpret_cast<uintptr_t>(a->q_init)) & 3)
        return fail(SSD_ERR_INVALID, "ssd_rollout_priority: q_env, q_inc, reward, carry, acc and q_init must be 4-byte aligned");
    if ((reinterpret_cast<uintptr_t>(a->t_index) | reinterpret_cast<uintptr_t>(a->actions) | reinterpret_cast<uintptr_t>(a->actions_inc) | reinterpret_cast<uintptr_t>(a->filled)) & 7)
        return fail(SSD_ERR_INVALID, "ssd_rollout_priority: t_index, actions, actions_inc and filled must be 8-byte aligned");
    if (a->n_segments < 0 || a->n_segments > SSD_PRIORITY_SEGMENTS_MAX) return fail(SSD_ERR_INVALID, "ssd_rollout_priority: n_segments outside 0 .. SSD_PRIORITY_SEGMENTS_MAX");
    if (a->n_segments) {                                                     // a priority per window of the stride grid
        const int T = a->t_slots - 1, L = a->win_len, s = a->seg_stride;
        if (L < 1 || L > T) return fail(SSD_ERR_INVALID, "ssd_rollout_priority: win_len outside 1 .. t_slots - 1");
        if (s < 1 || s > L) return fail(SSD_ERR_INVALID, "ssd_rollout_priority: seg_stride outside 1 .. win_len");
        if ((L + s - 1) / s > 8) return fail(SSD_ERR_INVALID, "ssd_rollout_priority: ceil(win_len / seg_stride) over 8");
        if (a->burn_in < 0 || a->burn_in >= L) return fail(SSD_ERR_INVALID, "ssd_rollout_priority: burn_in outside 0 .. win_len - 1");
        if (a->n_segments != (T - L + s - 1) / s + 1) return fail(SSD_ERR_INVALID, "ssd_rollout_priority: n_segments != ceil((T - win_len) / seg_stride) + 1");
    }
    launch_rollout_priority(a, (hipStream_t)stream);
    return launched();
}

int ssd_behaviour_stats(const ssd_behaviour_args* a, void* stream) {
    if (!a) return fail(SSD_ERR_INVALID, "ssd_behaviour_stats: null args");
    if (!a->actions || !a->actions_inc || !a->reward || !a->clean_num || !a->workspace || !a->acc)
        return fail(SSD_ERR_INVALID, "ssd_behaviour_stats: null member pointer");
    if (a->n_env < 1 || a->t_slots < 2) return fail(SSD_ERR_INVALID, "ssd_behaviour_stats: n_env >= 1, t_slots >= 2");
    if (a->n_agents < 1 || a->n_agents > SSD_MAX_AGENTS) return fail(SSD_ERR_INVALID, "ssd_behaviour_stats: n_agents outside 1 .. SSD_MAX_AGENTS");
    if (a->n_actions < 1 || a->n_actions > 16) return fail(SSD_ERR_INVALID, "ssd_behaviour_stats: n_actions outside 1 .. 16");
    if ((int64_t)a->t_slots * a->n_agents * a->n_agents > (int64_t)INT32_MAX)
        return fail(SSD_ERR_INVALID, "ssd_behaviour_stats: t_slots * n_agents^2 over INT32_MAX (32-bit index inside an env's block)");
    launch_behaviour_stats(a, (hipStream_t)stream);
    return launched();
}

int ssd_td_sim_loss(const ssd_td_loss_args* a, int32_t mode, void* stream) {
    if (!a || a->batch < 1 || a->t_slots < 2 || a->n_agents < 2 || a->n_agents > SSD_MAX_AGENTS || a->n_actions < 1 || a->sim_horizon < 1)
        return fail(SSD_ERR_INVALID, "bad argument");
    if ((int64_t)a->batch * a->t_slots * a->n_agents > SSD_ROWS32_MAX) return fail(SSD_ERR_INVALID, "ssd_td_sim_loss: batch * t_slots * n_agents over SSD_ROWS32_MAX");
    if (!a->reward || !a->clean_num || !a->terminated || !a->filled || !a->partials) return fail(SSD_ERR_INVALID, "null argument");
    if (mode && (!a->q_env || !a->q_inc || !a->tq_env || !a->tq_inc || !a->actions || !a->actions_inc || !a->avail || !a->dens || !a->dq_env || !a->dq_inc))
        return fail(SSD_ERR_INVALID, "null argument");
    if (!(a->seq_len > 0.f) || !(a->reward_scale != 0.f)) return fail(SSD_ERR_INVALID, "seq_len / reward_scale");
    if (mode && !(a->td_lambda >= 0.f && a->td_lambda <= 1.f)) return fail(SSD_ERR_INVALID, "ssd_td_sim_loss: td_lambda outside [0, 1]");
    launch_td_sim_loss(a, mode ? 1 : 0, (hipStream_t)stream);
    return launched();
}

// the edges the two refusal messages below name
static_assert(encoder_lds_bytes(36) <= kDefaultLdsLimit && encoder_lds_bytes(37) > kDefaultLdsLimit, "ssd_encoder's message names 3 .. 36");
static_assert(conv_leaky_lds_bytes(73) <= kDefaultLdsLimit && conv_leaky_lds_bytes(74) > kDefaultLdsLimit, "ssd_conv_leaky's message names 3 .. 73");
int ssd_encoder(const float* obs, int32_t rows, int32_t view_edge, int32_t conv_out, int32_t feat_out, const float* conv_w,
                const float* conv_b, const float* lin_w, const float* lin_b, float* out, int32_t out_stride, int32_t n_agents,
                int32_t agent_major, float* store_obs, int64_t store_env_stride, const int64_t* store_t, void* stream) {
    if (!obs || !conv_w || !conv_b || !lin_w || !lin_b || !out || rows < 1 || view_edge < 3) return fail(SSD_ERR_INVALID, "bad argument");
    if (conv_out != 6 || feat_out != 32) return fail(SSD_ERR_UNSUPPORTED, "ssd_encoder is instantiated for conv_out 6, obs_dim_net 32 (config/default.yaml:59-63)");
    if (encoder_lds_bytes(view_edge) > kDefaultLdsLimit)       // (before the storage checks: an accepted edge with a storage fault names the storage)
        return fail(SSD_ERR_INVALID, "ssd_encoder: the LDS staging of four windows of this view_edge exceeds the 64 KiB a launch may ask for (view_edge 3 .. 36)");
    if ((agent_major || store_obs) && (n_agents < 1 || rows % n_agents)) return fail(SSD_ERR_INVALID, "rows must be a multiple of n_agents");
    if (store_obs && !store_t) return fail(SSD_ERR_INVALID, "store_obs needs store_t");
    launch_encoder(obs, rows, view_edge, conv_w, conv_b, lin_w, lin_b, out, out_stride, n_agents, agent_major, store_obs,
                   (long)store_env_stride, store_t, (hipStream_t)stream);
    return launched();
}

int ssd_conv_leaky(const float* obs, int32_t rows, int32_t view_edge, int32_t conv_out, const float* conv_w, const float* conv_b,
                   float* out, int32_t n_agents, int32_t agent_major, float* store_obs, int64_t store_env_stride,
                   const int64_t* store_t, void* stream) {
    if (!obs || !conv_w || !conv_b || !out || rows < 1 || view_edge < 3 || n_agents < 1 || rows % n_agents) return fail(SSD_ERR_INVALID, "bad argument");
    if (conv_out != 6) return fail(SSD_ERR_UNSUPPORTED, "ssd_conv_leaky is instantiated for conv_out 6 (config/default.yaml:59)");
    if (conv_leaky_lds_bytes(view_edge) > kDefaultLdsLimit)
        return fail(SSD_ERR_INVALID, "ssd_conv_leaky: the LDS staging of a window of this view_edge exceeds the 64 KiB a launch may ask for (view_edge 3 .. 73)");
    if (store_obs && !store_t) return fail(SSD_ERR_INVALID, "store_obs needs store_t");
    launch_conv_leaky(obs, rows, view_edge, conv_w, conv_b, out, n_agents, agent_major, store_obs, (long)store_env_stride, store_t,
                      (hipStream_t)stream);
    return launched();
}

int ssd_store_step_launch(const ssd_store_step* a, void* stream) {
    if (!a || !a->t_index || a->n_env < 1 || a->n_agents < 1 || a->t_slots < 1) return fail(SSD_ERR_INVALID, "bad argument");
    if (a->next_t_out && a->next_t_out == a->t_index) return fail(SSD_ERR_INVALID, "next_t_out must not alias t_index");
    if ((a->prev_reward || a->ep_return) && !a->reward) return fail(SSD_ERR_INVALID, "prev_reward / ep_return need reward");
    launch_store_step(a, (hipStream_t)stream);
    return launched();
}

int ssd_store_hidden(const ssd_store_hidden_args* a, void* stream) {
    if (!a) return fail(SSD_ERR_INVALID, "ssd_store_hidden: null args");
    if (!a->t_index || !a->h_env || !a->h_inc || !a->dst) return fail(SSD_ERR_INVALID, "ssd_store_hidden: null member pointer");
    if (a->n_env < 1 || a->n_agents < 1 || a->t_slots < 1) return fail(SSD_ERR_INVALID, "ssd_store_hidden: n_env, n_agents and t_slots must be at least 1");
    if ((reinterpret_cast<uintptr_t>(a->dst) | reinterpret_cast<uintptr_t>(a->h_env) | reinterpret_cast<uintptr_t>(a->h_inc)) & 15)
        return fail(SSD_ERR_INVALID, "ssd_store_hidden: h_env, h_inc and dst must be 16-byte aligned");
    if (a->src_agent_stride < 0 || a->src_env_stride < 0 || (a->src_agent_stride & 3) || (a->src_env_stride & 3))
        return fail(SSD_ERR_INVALID, "ssd_store_hidden: source strides must be non-negative multiples of 4 elements");
    if ((int64_t)a->n_env * a->n_agents >= (int64_t)1 << 34) return fail(SSD_ERR_INVALID, "ssd_store_hidden: n_env * n_agents over 2^34");
    launch_store_hidden(a, (hipStream_t)stream);
    return launched();
}

int ssd_gru_gates(const float* gi, const float* gh, float* h, int32_t rows, int32_t hidden, void* stream) {
    if (!gi || !gh || !h || rows < 1 || hidden < 1) return fail(SSD_ERR_INVALID, "bad argument");
    launch_gru_gates(gi, gh, h, rows, hidden, (hipStream_t)stream);
    return launched();
}

int ssd_gru_gates_fwd(const float* gi, const float* gh, const float* h, float* h_new, float* rzn, int32_t rows, int32_t hidden, void* stream) {
    if (!gi || !gh || !h || !h_new || !rzn || rows < 1 || hidden < 1) return fail(SSD_ERR_INVALID, "bad argument");
    launch_gru_fwd_train(gi, gh, h, h_new, rzn, rows, hidden, (hipStream_t)stream);
    return launched();
}

int ssd_gru_gates_bwd(const float* dh_new, const float* rzn, const float* gh, const float* h, float* d_gi, float* d_gh, float* dh_prev,
                      int32_t rows, int32_t hidden, void* stream) {
    if (!dh_new || !rzn || !gh || !h || !d_gi || !d_gh || !dh_prev || rows < 1 || hidden < 1) return fail(SSD_ERR_INVALID, "bad argument");
    launch_gru_bwd(dh_new, rzn, gh, h, d_gi, d_gh, dh_prev, rows, hidden, (hipStream_t)stream);
    return launched();
}

int ssd_dueling_pick(const float* av, int32_t rows, int32_t n_actions, const uint8_t* avail, const float* epsilon, const int64_t* step,
                     uint32_t seed, int32_t n_agents, int32_t batch, int32_t pairs, int64_t* actions, float* q_out, uint32_t env_id_base,
                     void* stream) {
    if (!av || !epsilon || !step || !actions || rows < 1 || n_actions < 1 || n_agents < 1 || batch < 1) return fail(SSD_ERR_INVALID, "bad argument");
    if (rows != (pairs ? n_agents * batch * n_agents : n_agents * batch)) return fail(SSD_ERR_INVALID, "rows must be n*B (or n*B*n for pairs)");
    // the availability mask is gathered into 16 bits (avail_to_bits) and the draw's pick walks one 32-bit word
    if (n_actions > 16) return fail(SSD_ERR_UNSUPPORTED, "ssd_dueling_pick: n_actions must be 1 .. 16");
    launch_dueling_pick(av, rows, n_actions, avail, epsilon, step, seed, n_agents, batch, pairs, actions, q_out, env_id_base, (hipStream_t)stream);
    return launched();
}

static bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// The argument checks of the six ssd_gru_seq_* exports, written once per direction.  `who`: the calling export, first in every
// message.  min_parts: the smallest n_parts the export admits -- 1 for the _parts forms, 0 (one time-major tensor behind a
// one-element table) for the _h0 forms and the time-major pair, which hands its single pointers over as such tables.  h0_parts
// is looked at only with with_h0.  SSD_OK or SSD_ERR_INVALID.
static int gru_seq_fwd_check(const char* who, int min_parts, bool with_h0, const float* const* gi_parts, int32_t n_parts, const float* const* wh_parts,
                             const float* const* bh_parts, int32_t n_wparts, const float* const* h0_parts, int64_t h0_set_stride, int64_t h0_row_stride,
                             const float* hs, const float* rzn, const float* ghn, int32_t T, int32_t G, int32_t B) {
    const int np = n_parts < 1 ? 1 : n_parts;
    if (!gi_parts || n_parts < min_parts || n_parts > 4 || !wh_parts || !bh_parts || n_wparts < 1 || n_wparts > 4 || (with_h0 && !h0_parts) || !hs || T < 1 ||
        G < 1 || G % np || G % n_wparts || B < 1 || (!rzn) != (!ghn))
        return fail(SSD_ERR_INVALID, "%s: bad argument", who);
    for (int k = 0; k < n_wparts; ++k)
        if (!wh_parts[k] || !bh_parts[k] || !al16(wh_parts[k]) || !al16(bh_parts[k])) return fail(SSD_ERR_INVALID, "%s: weight parts must be non-null and 16-byte aligned", who);
    if (B % 16) return fail(SSD_ERR_INVALID, "%s: B must be a multiple of 16 (pad the sequences)", who);
    for (int k = 0; k < np; ++k) {
        if (!gi_parts[k] || !al16(gi_parts[k])) return fail(SSD_ERR_INVALID, "%s: gi parts must be non-null and 16-byte aligned", who);
        if (with_h0 && (!h0_parts[k] || !al16(h0_parts[k]))) return fail(SSD_ERR_INVALID, "%s: h0 parts must be non-null and 16-byte aligned", who);
    }
    if (with_h0 && (h0_set_stride < 0 || h0_row_stride < 0 || (h0_set_stride & 3) || (h0_row_stride & 3)))
        return fail(SSD_ERR_INVALID, "%s: h0 strides must be non-negative multiples of 4 elements", who);
    if (!al16(hs) || !al16(rzn) || !al16(ghn)) return fail(SSD_ERR_INVALID, "%s: tensors must be 16-byte aligned", who);
    return SSD_OK;
}
static int gru_seq_bwd_check(const char* who, int min_parts, const float* const* dhs_parts, const float* hs, const float* rzn, const float* ghn,
                             const float* const* wh_parts, int32_t n_wparts, float* const* d_gi_parts, int32_t n_parts, const float* dgh, const float* d_wh,
                             const float* d_bh_part, int32_t T, int32_t G, int32_t G_grad, int32_t B) {
    const int np = n_parts < 1 ? 1 : n_parts;
    if (!dhs_parts || !hs || !rzn || !ghn || !wh_parts || n_wparts < 1 || n_wparts > 4 || !d_gi_parts || n_parts < min_parts || n_parts > 4 || !dgh || !d_wh ||
        !d_bh_part || T < 1 || G < 1 || G % np || G % n_wparts || B < 1 || G_grad < 1 || G_grad > G || G_grad % (G / np))
        return fail(SSD_ERR_INVALID, "%s: bad argument", who);
    for (int k = 0; k * (G / np) < G_grad; ++k)
        if (!dhs_parts[k] || !al16(dhs_parts[k]) || !d_gi_parts[k] || !al16(d_gi_parts[k]))
            return fail(SSD_ERR_INVALID, "%s: dhs and d_gi parts of the sets with a gradient must be non-null and 16-byte aligned", who);
    for (int k = 0; k < n_wparts; ++k)
        if (!wh_parts[k] || !al16(wh_parts[k])) return fail(SSD_ERR_INVALID, "%s: weight parts must be non-null and 16-byte aligned", who);
    if (B % 16) return fail(SSD_ERR_INVALID, "%s: B must be a multiple of 16 (pad the sequences)", who);
    if (!al16(hs) || !al16(rzn) || !al16(ghn) || !al16(dgh)) return fail(SSD_ERR_INVALID, "%s: tensors must be 16-byte aligned", who);
    return SSD_OK;
}

int ssd_gru_seq_fwd(const float* gi, const float* wh, const float* bh, float* hs, float* rzn, float* ghn, int32_t T, int32_t G, int32_t B,
                    void* stream) {
    if (int rc = gru_seq_fwd_check("ssd_gru_seq_fwd", 0, false, &gi, 0, &wh, &bh, 1, nullptr, 0, 0, hs, rzn, ghn, T, G, B)) return rc;
    launch_gru_seq_fwd(&gi, 0, &wh, &bh, 1, hs, rzn, ghn, T, G, B, (hipStream_t)stream);
    return launched();
}
int ssd_gru_seq_fwd_parts(const float* const* gi_parts, int32_t n_parts, const float* const* wh_parts, const float* const* bh_parts, int32_t n_wparts,
                          float* hs, float* rzn, float* ghn, int32_t T, int32_t G, int32_t B, void* stream) {
    if (int rc = gru_seq_fwd_check("ssd_gru_seq_fwd_parts", 1, false, gi_parts, n_parts, wh_parts, bh_parts, n_wparts, nullptr, 0, 0, hs, rzn, ghn, T, G, B)) return rc;
    launch_gru_seq_fwd(gi_parts, n_parts, wh_parts, bh_parts, n_wparts, hs, rzn, ghn, T, G, B, (hipStream_t)stream);
    return launched();
}
int ssd_gru_seq_fwd_h0(const float* const* gi_parts, int32_t n_parts, const float* const* wh_parts, const float* const* bh_parts, int32_t n_wparts,
                       const float* const* h0_parts, int64_t h0_set_stride, int64_t h0_row_stride, float* hs, float* rzn, float* ghn, int32_t T, int32_t G,
                       int32_t B, void* stream) {
    if (int rc = gru_seq_fwd_check("ssd_gru_seq_fwd_h0", 0, true, gi_parts, n_parts, wh_parts, bh_parts, n_wparts, h0_parts, h0_set_stride, h0_row_stride, hs, rzn,
                                   ghn, T, G, B))
        return rc;
    launch_gru_seq_fwd(gi_parts, n_parts, wh_parts, bh_parts, n_wparts, hs, rzn, ghn, T, G, B, (hipStream_t)stream, h0_parts, (long)h0_set_stride,
                       (long)h0_row_stride);
    return launched();
}

int ssd_gru_seq_bwd(const float* dhs, const float* hs, const float* rzn, const float* ghn, const float* wh, float* d_gi, float* dgh,
                    float* d_wh, float* d_bh_part, int32_t T, int32_t G, int32_t B, void* stream) {
    if (int rc = gru_seq_bwd_check("ssd_gru_seq_bwd", 0, &dhs, hs, rzn, ghn, &wh, 1, &d_gi, 0, dgh, d_wh, d_bh_part, T, G, G, B)) return rc;
    launch_gru_seq_bwd(&dhs, hs, rzn, ghn, &wh, 1, &d_gi, 0, dgh, d_wh, d_bh_part, T, G, G, B, (hipStream_t)stream);
    return launched();
}
int ssd_gru_seq_bwd_parts(const float* const* dhs_parts, const float* hs, const float* rzn, const float* ghn, const float* const* wh_parts, int32_t n_wparts,
                          float* const* d_gi_parts, int32_t n_parts, float* dgh, float* d_wh, float* d_bh_part, int32_t T, int32_t G, int32_t G_grad, int32_t B,
                          void* stream) {
    if (int rc = gru_seq_bwd_check("ssd_gru_seq_bwd_parts", 1, dhs_parts, hs, rzn, ghn, wh_parts, n_wparts, d_gi_parts, n_parts, dgh, d_wh, d_bh_part, T, G, G_grad, B))
        return rc;
    launch_gru_seq_bwd(dhs_parts, hs, rzn, ghn, wh_parts, n_wparts, d_gi_parts, n_parts, dgh, d_wh, d_bh_part, T, G, G_grad, B, (hipStream_t)stream);
    return launched();
}
int ssd_gru_seq_bwd_h0(const float* const* dhs_parts, const float* hs, const float* rzn, const float* ghn, const float* const* wh_parts, int32_t n_wparts,
                       float* const* d_gi_parts, int32_t n_parts, float* dgh, float* d_wh, float* d_bh_part, int32_t T, int32_t G, int32_t G_grad, int32_t B,
                       void* stream) {
    if (int rc = gru_seq_bwd_check("ssd_gru_seq_bwd_h0", 0, dhs_parts, hs, rzn, ghn, wh_parts, n_wparts, d_gi_parts, n_parts, dgh, d_wh, d_bh_part, T, G, G_grad, B))
        return rc;
    launch_gru_seq_bwd(dhs_parts, hs, rzn, ghn, wh_parts, n_wparts, d_gi_parts, n_parts, dgh, d_wh, d_bh_part, T, G, G_grad, B, (hipStream_t)stream, true);
    return launched();
}

int ssd_bias_bmm_fwd(const float* x, const float* w, const float* b, float* y, int32_t n, int32_t rows, int32_t in, int32_t out, void* stream) {
    if (!x || !w || !b || !y || n < 1 || rows < 1 || in < 1 || out < 1) return fail(SSD_ERR_INVALID, "bad argument");
    if (launch_bias_bmm_fwd(x, w, b, y, n, rows, in, out, (hipStream_t)stream)) return fail(SSD_ERR_UNSUPPORTED, "ssd_bias_bmm_fwd: a weight / operand set of 2^30 elements or more");
    return launched();
}
int ssd_bias_bmm_leaky_fwd(const float* x, const float* w, const float* b, float* y, int32_t n, int32_t rows, int32_t in, int32_t out, void* stream) {
    if (!x || !w || !b || !y || n < 1 || rows < 1 || in < 1 || out < 1) return fail(SSD_ERR_INVALID, "bad argument");
    if (launch_bias_bmm_fwd(x, w, b, y, n, rows, in, out, (hipStream_t)stream, 1)) return fail(SSD_ERR_UNSUPPORTED, "ssd_bias_bmm_leaky_fwd: a weight / operand set of 2^30 elements or more");
    return launched();
}
int ssd_bias_bmm_leaky_bwd(const float* g, const float* y, const float* x, const float* w, float* dx, float* dw, float* db, const float* slope_of,
                           int32_t n, int32_t rows, int32_t in, int32_t out, void* stream) {
    if (!g || !y || n < 1 || rows < 1 || in < 1 || out < 1) return fail(SSD_ERR_INVALID, "bad argument");
    if ((dx && !w) || ((dw || db) && !x) || (slope_of && !dx)) return fail(SSD_ERR_INVALID, "dx needs w, dw / db need x, slope_of needs dx");
    if (launch_bias_bmm_bwd(g, x, w, dx, dw, db, slope_of, n, rows, in, out, (hipStream_t)stream, 0, 0, y)) return fail(SSD_ERR_UNSUPPORTED, "ssd_bias_bmm_leaky_bwd: an operand set of 2^30 elements or more");
    return launched();
}
int ssd_bias_bmm_bwd(const float* g, const float* x, const float* w, float* dx, float* dw, float* db, const float* slope_of, int32_t n,
                     int32_t rows, int32_t in, int32_t out, void* stream) {
    if (!g || n < 1 || rows < 1 || in < 1 || out < 1) return fail(SSD_ERR_INVALID, "bad argument");
    if ((dx && !w) || ((dw || db) && !x) || (slope_of && !dx)) return fail(SSD_ERR_INVALID, "dx needs w, dw / db need x, slope_of needs dx");
    if (launch_bias_bmm_bwd(g, x, w, dx, dw, db, slope_of, n, rows, in, out, (hipStream_t)stream)) return fail(SSD_ERR_UNSUPPORTED, "ssd_bias_bmm_bwd: an operand set of 2^30 elements or more");
    return launched();
}

int ssd_dueling_head_fwd(const float* y, float* q, int32_t n, int32_t T, int32_t B, int32_t inner, int32_t K, void* stream) {
    if (!y || !q || n < 1 || T < 1 || B < 1 || inner < 1 || K < 1 || K > 15) return fail(SSD_ERR_INVALID, "bad argument");
    launch_dueling_q(y, y + K, q, nullptr, nullptr, nullptr, n, T, B, inner, K, (hipStream_t)stream, K + 1, 1, nullptr);
    return launched();
}
int ssd_dueling_head_bwd(const float* dq, float* dy, float* gs, int32_t n, int32_t T, int32_t B, int32_t inner, int32_t K, void* stream) {
    if (!dq || !dy || n < 1 || T < 1 || B < 1 || inner < 1 || K < 1 || K > 15) return fail(SSD_ERR_INVALID, "bad argument");
    launch_dueling_q(nullptr, nullptr, nullptr, dq, dy, dy + K, n, T, B, inner, K, (hipStream_t)stream, K + 1, 1, gs);
    return launched();
}
int ssd_bias_bmm2_fwd(const float* x1, const float* x2, const float* w, const float* b, float* y, int32_t n, int32_t rows, int32_t in1, int32_t in2,
                      int32_t out, int32_t x1_div, int32_t x2_shared, void* stream) {
    if (!x1 || !x2 || !w || !b || !y || n < 1 || rows < 1 || in1 < 1 || in2 < 1 || out < 1) return fail(SSD_ERR_INVALID, "bad argument");
    const int rc = launch_bias_bmm2_fwd(x1, x2, w, b, y, n, rows, in1, in2, out, x1_div, x2_shared, (hipStream_t)stream);
    if (rc == -3) return fail(SSD_ERR_INVALID, "ssd_bias_bmm2_fwd: in1 a multiple of 16, rows a multiple of x1_div >= 1");
    if (rc) return fail(SSD_ERR_UNSUPPORTED, "ssd_bias_bmm2_fwd: a weight / operand set of 2^30 elements or more");
    return launched();
}
int ssd_bias_bmm2_bwd_w(const float* g, const float* x1, const float* x2, float* dw, float* db, int32_t n, int32_t rows, int32_t in1, int32_t in2,
                        int32_t out, int32_t x1_div, int32_t x2_shared, void* stream) {
    if (!g || !x1 || !x2 || (!dw && !db) || n < 1 || rows < 1 || in1 < 1 || in2 < 1 || out < 1) return fail(SSD_ERR_INVALID, "bad argument");
    const int rc = launch_bias_bmm_bwd(g, x1, nullptr, nullptr, dw, db, nullptr, n, rows, in1 + in2, out, (hipStream_t)stream, 0, 0, nullptr, x2, in1, x1_div,
                                       x2_shared, 0);
    if (rc == -3) return fail(SSD_ERR_INVALID, "ssd_bias_bmm2_bwd_w: in1 a multiple of 16, rows a multiple of x1_div >= 1");
    if (rc) return fail(SSD_ERR_UNSUPPORTED, "ssd_bias_bmm2_bwd_w: an operand set of 2^30 elements or more");
    return launched();
}
int ssd_bias_bmm_bwd_x(const float* g, const float* w, float* dx, int32_t n, int32_t rows, int32_t in, int32_t out, int64_t w_set, void* stream) {
    if (!g || !w || !dx || n < 1 || rows < 1 || in < 1 || out < 1 || w_set < (int64_t)in * out) return fail(SSD_ERR_INVALID, "bad argument");
    if (launch_bias_bmm_bwd(g, nullptr, w, dx, nullptr, nullptr, nullptr, n, rows, in, out, (hipStream_t)stream, 0, 0, nullptr, nullptr, 0, 1, 0, (long)w_set))
        return fail(SSD_ERR_UNSUPPORTED, "ssd_bias_bmm_bwd_x: an operand set of 2^30 elements or more");
    return launched();
}
int ssd_bias_bmm_pair_fwd(const float* x_a, const float* x2_a, const float* w_a, const float* b_a, float* y_a, int32_t n_a, const float* x_b,
                          const float* x2_b, const float* w_b, const float* b_b, float* y_b, int32_t n_b, int32_t rows, int32_t in1, int32_t in2,
                          int32_t out, int32_t x1_div, int32_t x2_shared, int32_t leaky, void* stream) {
    if (!x_a || !w_a || !b_a || !y_a || !x_b || !w_b || !b_b || !y_b) return fail(SSD_ERR_INVALID, "ssd_bias_bmm_pair_fwd: a null operand of either group");
    if (n_a < 1 || n_b < 1) return fail(SSD_ERR_INVALID, "ssd_bias_bmm_pair_fwd: both groups need a set count >= 1");
    if (rows < 1 || in1 < 1 || in2 < 0 || out < 1) return fail(SSD_ERR_INVALID, "ssd_bias_bmm_pair_fwd: bad argument");
    if ((in2 > 0) != (x2_a != nullptr) || (in2 > 0) != (x2_b != nullptr))
        return fail(SSD_ERR_INVALID, "ssd_bias_bmm_pair_fwd: in2 > 0 needs the second source of both groups, in2 == 0 neither");
    if ((long)n_a + n_b > 65535) return fail(SSD_ERR_UNSUPPORTED, "ssd_bias_bmm_pair_fwd: more than 65535 weight sets in one grid");
    const int rc = launch_bias_bmm_pair_fwd(x_a, x2_a, w_a, b_a, y_a, n_a, x_b, x2_b, w_b, b_b, y_b, n_b, rows, in1, in2, out, x1_div, x2_shared, leaky != 0,
                                            (hipStream_t)stream);
    if (rc == -3)
        return fail(SSD_ERR_INVALID, "ssd_bias_bmm_pair_fwd: rows a multiple of x1_div >= 1; in1 a multiple of 16 unless in2 is no multiple of 4");
    if (rc) return fail(SSD_ERR_UNSUPPORTED, "ssd_bias_bmm_pair_fwd: a weight / operand set of 2^30 elements or more");
    return launched();
}
int ssd_dueling_head_pair_fwd(const float* y_a, float* q_a, int32_t n_a, const float* y_b, float* q_b, int32_t n_b, int32_t T, int32_t B, int32_t inner,
                              int32_t K, void* stream) {
    if (!y_a || !q_a || !y_b || !q_b) return fail(SSD_ERR_INVALID, "ssd_dueling_head_pair_fwd: a null operand of either group");
    if (n_a < 1 || n_b < 1) return fail(SSD_ERR_INVALID, "ssd_dueling_head_pair_fwd: both groups need a set count >= 1");
    if (T < 1 || B < 1 || inner < 1 || K < 1 || K > 15) return fail(SSD_ERR_INVALID, "ssd_dueling_head_pair_fwd: bad argument");
    launch_dueling_q(y_a, y_a + K, q_a, nullptr, nullptr, nullptr, n_a, T, B, inner, K, (hipStream_t)stream, K + 1, 1, nullptr, y_b, y_b + K, q_b, n_b);
    return launched();
}
int ssd_fc1_rows_fwd(const float* feat_a, const float* feat_b, const float* tail, const float* act, float* x_env_a, float* x_inc_a, float* x_env_b,
                     float* x_inc_b, int32_t B, int32_t T, int32_t n, int32_t feat_w, int32_t tail_w, int32_t act_w, void* stream) {
    if (!feat_a || !act || !x_env_a || !x_inc_a) return fail(SSD_ERR_INVALID, "ssd_fc1_rows_fwd: a null operand of the first net");
    if ((feat_b != nullptr) != (x_env_b != nullptr) || (feat_b != nullptr) != (x_inc_b != nullptr))
        return fail(SSD_ERR_INVALID, "ssd_fc1_rows_fwd: the second net's features and both its outputs come together or not at all");
    if (B < 1 || T < 1 || n < 1 || feat_w < 1 || tail_w < 0 || act_w < 1) return fail(SSD_ERR_INVALID, "ssd_fc1_rows_fwd: bad argument");
    if ((tail_w > 0) != (tail != nullptr)) return fail(SSD_ERR_INVALID, "ssd_fc1_rows_fwd: tail_w > 0 needs tail, tail_w == 0 none");
    if ((int64_t)B * T * n * ((int64_t)feat_w + tail_w + act_w) >= ((int64_t)1 << 40)) return fail(SSD_ERR_UNSUPPORTED, "ssd_fc1_rows_fwd: 2^40 elements or more");
    launch_fc1_rows(feat_a, feat_b, tail, act, x_env_a, x_inc_a, x_env_b, x_inc_b, B, T, n, feat_w, tail_w, act_w, (hipStream_t)stream);
    return launched();
}
int ssd_fc1_rows_bwd(const float* d_x_env, const float* d_x_inc, float* d_feat, int32_t B, int32_t T, int32_t n, int32_t feat_w, int32_t tail_w, int32_t act_w,
                     int32_t d_feat_stride, void* stream) {
    if (!d_x_env || !d_x_inc || !d_feat) return fail(SSD_ERR_INVALID, "ssd_fc1_rows_bwd: a null operand");
    if (B < 1 || T < 1 || n < 1 || feat_w < 1 || tail_w < 0 || act_w < 1) return fail(SSD_ERR_INVALID, "ssd_fc1_rows_bwd: bad argument");
    if (d_feat_stride < feat_w) return fail(SSD_ERR_INVALID, "ssd_fc1_rows_bwd: d_feat_stride below feat_w");
    if ((int64_t)B * T * n * ((int64_t)feat_w + tail_w + act_w) >= ((int64_t)1 << 40)) return fail(SSD_ERR_UNSUPPORTED, "ssd_fc1_rows_bwd: 2^40 elements or more");
    launch_fc1_rows_bwd(d_x_env, d_x_inc, d_feat, B, T, n, feat_w, tail_w, act_w, d_feat_stride, (hipStream_t)stream);
    return launched();
}
// include/ssd_hip_reward.h: the reward model over a finished rollout (csrc/ssd_social_reward.hip)
int ssd_social_reward(int32_t model, const float* reward, float* shaped, double* acc, int32_t n_env, int32_t t_slots, int32_t n_agents,
                      int32_t src_env_stride, int32_t src_slot_stride, int32_t dst_env_stride, int32_t dst_slot_stride, float p0, float p1, float p2,
                      void* stream) {
    if (!reward || !shaped) return fail(SSD_ERR_INVALID, "ssd_social_reward: a null reward or shaped");
    if (model != SSD_REWARD_IA && model != SSD_REWARD_PROSOCIAL) return fail(SSD_ERR_INVALID, "ssd_social_reward: model must be SSD_REWARD_IA (1) or SSD_REWARD_PROSOCIAL (2)");
    if (n_env < 1) return fail(SSD_ERR_INVALID, "ssd_social_reward: n_env must be >= 1");
    if (t_slots < 2) return fail(SSD_ERR_INVALID, "ssd_social_reward: t_slots must be >= 2 (one slot and the bootstrap slot)");
    if (n_agents < 2 || n_agents > SSD_MAX_AGENTS) return fail(SSD_ERR_INVALID, "ssd_social_reward: n_agents out of range (2..10)");
    if (src_slot_stride < n_agents || dst_slot_stride < n_agents) return fail(SSD_ERR_INVALID, "ssd_social_reward: a slot stride below n_agents");
    if (src_env_stride < (int64_t)t_slots * src_slot_stride || dst_env_stride < (int64_t)t_slots * dst_slot_stride)
        return fail(SSD_ERR_INVALID, "ssd_social_reward: an env stride below t_slots * slot_stride");
    if (!(p0 >= 0.0f) || !(p1 >= 0.0f) || !std::isfinite(p0) || !std::isfinite(p1))
        return fail(SSD_ERR_INVALID, "ssd_social_reward: p0 and p1 must be finite and >= 0");
    if (model == SSD_REWARD_IA && !(p2 >= 0.0f && p2 < 1.0f)) return fail(SSD_ERR_INVALID, "ssd_social_reward: the decay p2 must lie in [0, 1)");
    const int64_t src_ext = (int64_t)(n_env - 1) * src_env_stride + (int64_t)(t_slots - 1) * src_slot_stride + n_agents;
    const int64_t dst_ext = (int64_t)(n_env - 1) * dst_env_stride + (int64_t)(t_slots - 1) * dst_slot_stride + n_agents;
    if (src_ext > INT32_MAX || dst_ext > INT32_MAX) return fail(SSD_ERR_INVALID, "ssd_social_reward: an extent past 2^31 - 1 elements");
    if (((uintptr_t)reward | (uintptr_t)shaped) & 3) return fail(SSD_ERR_INVALID, "ssd_social_reward: reward or shaped is not 4-byte aligned");
    if ((uintptr_t)acc & 7) return fail(SSD_ERR_INVALID, "ssd_social_reward: acc (f64) is not 8-byte aligned");
    if ((uintptr_t)shaped < (uintptr_t)reward + 4 * (uintptr_t)src_ext && (uintptr_t)reward < (uintptr_t)shaped + 4 * (uintptr_t)dst_ext)
        return fail(SSD_ERR_INVALID, "ssd_social_reward: shaped and reward must be distinct buffers that do not overlap");
    launch_social_reward(model, reward, shaped, acc, n_env, t_slots, n_agents, src_env_stride, src_slot_stride, dst_env_stride, dst_slot_stride, p0, p1, p2,
                         (hipStream_t)stream);
    return launched();
}
// include/ssd_hip_tie.h: heads shared across agents (csrc/ssd_agent_tie.hip).  Everything is checked on the host table.
int ssd_tie_agent_grads(float* flat, int64_t total, const int64_t* jobs_host, const int64_t* jobs_dev, int32_t n_jobs, void* stream) {
    if (n_jobs < 0 || n_jobs > SSD_ADAM_MAX_JOBS) return fail(SSD_ERR_INVALID, "ssd_tie_agent_grads: n_jobs outside 0 .. SSD_ADAM_MAX_JOBS");
    if (n_jobs == 0) return SSD_OK;
    if (!flat || !jobs_host || !jobs_dev) return fail(SSD_ERR_INVALID, "ssd_tie_agent_grads: a null flat, jobs_host or jobs_dev");
    if ((uintptr_t)flat & 3) return fail(SSD_ERR_INVALID, "ssd_tie_agent_grads: flat is not 4-byte aligned");
    if (total < 1 || total > (int64_t)INT32_MAX) return fail(SSD_ERR_INVALID, "ssd_tie_agent_grads: total outside 1 .. 2^31 - 1");
    int64_t end = 0, max_inner = 0;
    for (int32_t k = 0; k < n_jobs; ++k) {
        const int64_t offset = jobs_host[3 * k], copies = jobs_host[3 * k + 1], inner = jobs_host[3 * k + 2];
        if (copies < 2 || copies > SSD_MAX_AGENTS) return fail(SSD_ERR_INVALID, "ssd_tie_agent_grads: copies outside 2 .. SSD_MAX_AGENTS");
        if (inner < 1) return fail(SSD_ERR_INVALID, "ssd_tie_agent_grads: inner must be >= 1");
        if (offset < 0 || offset > total || inner > (total - offset) / copies) return fail(SSD_ERR_INVALID, "ssd_tie_agent_grads: an extent past total");
        if (offset < end) return fail(SSD_ERR_INVALID, "ssd_tie_agent_grads: jobs overlap or do not ascend");
        end = offset + copies * inner;
        if (inner > max_inner) max_inner = inner;
    }
    launch_tie_agent_grads(flat, jobs_dev, n_jobs, (long)max_inner, (hipStream_t)stream);
    return launched();
}
int ssd_agent_spread(const int64_t* jobs_host, const int64_t* jobs_dev, int32_t n_jobs, double* out, void* stream) {
    if (n_jobs < 0 || n_jobs > SSD_ADAM_MAX_JOBS) return fail(SSD_ERR_INVALID, "ssd_agent_spread: n_jobs outside 0 .. SSD_ADAM_MAX_JOBS");
    if (n_jobs == 0) return SSD_OK;
    if (!jobs_host || !jobs_dev || !out) return fail(SSD_ERR_INVALID, "ssd_agent_spread: a null jobs_host, jobs_dev or out");
    if ((uintptr_t)out & 7) return fail(SSD_ERR_INVALID, "ssd_agent_spread: out (f64) is not 8-byte aligned");
    for (int32_t k = 0; k < n_jobs; ++k) {
        const int64_t address = jobs_host[3 * k], copies = jobs_host[3 * k + 1], inner = jobs_host[3 * k + 2];
        if (address == 0 || (address & 3)) return fail(SSD_ERR_INVALID, "ssd_agent_spread: an address that is null or not 4-byte aligned");
        if (copies < 2 || copies > SSD_MAX_AGENTS) return fail(SSD_ERR_INVALID, "ssd_agent_spread: copies outside 2 .. SSD_MAX_AGENTS");
        if (inner < 1 || inner > (int64_t)INT32_MAX / copies) return fail(SSD_ERR_INVALID, "ssd_agent_spread: inner outside 1 .. (2^31 - 1) / copies");
    }
    launch_agent_spread(jobs_dev, n_jobs, out, (hipStream_t)stream);
    return launched();
}
// include/ssd_hip_mix.h: the VDN mixer of the env head (csrc/ssd_team_mix.hip), behind ssd_td_sim_loss(args, 1) on the same struct
int ssd_team_td(const ssd_td_loss_args* a, void* stream) {
    if (!a) return fail(SSD_ERR_INVALID, "ssd_team_td: null args");
    if (a->batch < 1 || a->t_slots < 2 || a->n_actions < 1) return fail(SSD_ERR_INVALID, "ssd_team_td: batch >= 1, t_slots >= 2, n_actions >= 1");
    if (a->n_agents < 2 || a->n_agents > SSD_MAX_AGENTS) return fail(SSD_ERR_INVALID, "ssd_team_td: n_agents outside 2 .. SSD_MAX_AGENTS");
    if ((int64_t)a->batch * a->t_slots * a->n_agents > SSD_ROWS32_MAX) return fail(SSD_ERR_INVALID, "ssd_team_td: batch * t_slots * n_agents over SSD_ROWS32_MAX");
    if (!a->q_env || !a->tq_env || !a->actions || !a->actions_inc || !a->avail || !a->reward || !a->terminated || !a->filled || !a->dens || !a->dq_env
        || !a->partials)
        return fail(SSD_ERR_INVALID, "ssd_team_td: null member pointer (q_env, tq_env, actions, actions_inc, avail, reward, terminated, filled, dens, dq_env, partials)");
    if ((reinterpret_cast<uintptr_t>(a->q_env) | reinterpret_cast<uintptr_t>(a->tq_env) | reinterpret_cast<uintptr_t>(a->actions) | reinterpret_cast<uintptr_t>(a->actions_inc)
         | reinterpret_cast<uintptr_t>(a->avail) | reinterpret_cast<uintptr_t>(a->reward) | reinterpret_cast<uintptr_t>(a->filled) | reinterpret_cast<uintptr_t>(a->dens)
         | reinterpret_cast<uintptr_t>(a->dq_env) | reinterpret_cast<uintptr_t>(a->partials)) & 3)
        return fail(SSD_ERR_INVALID, "ssd_team_td: an operand is not 4-byte aligned (q_env, tq_env, actions, actions_inc, avail, reward, filled, dens, dq_env, partials)");
    if (!(a->seq_len > 0.f) || !(a->reward_scale != 0.f)) return fail(SSD_ERR_INVALID, "ssd_team_td: seq_len <= 0 or reward_scale == 0");
    if (!unit_interval(a->td_lambda)) return fail(SSD_ERR_INVALID, "ssd_team_td: td_lambda outside [0, 1]");
    launch_team_td(a, (hipStream_t)stream);
    return launched();
}
int ssd_bmm_reserve_scratch(void* stream) {
    if (!bmm_scratch((hipStream_t)stream)) return fail(SSD_ERR_DEVICE, "ssd_bmm_reserve_scratch: allocation failed (inside a stream capture?)");
    return SSD_OK;
}
int ssd_set_learner_precision(int32_t precision) {
    if (precision != 1 && precision != 2) return fail(SSD_ERR_INVALID, "ssd_set_learner_precision: 1 (bf16) or 2 (f32)");
    set_learner_precision(precision);
    return SSD_OK;
}
int ssd_learner_precision(void) { return learner_precision(); }
int ssd_conv_wgrad_partial_rows(int32_t rows) { return rows < 1 ? 0 : conv_wgrad_partial_rows(rows); }
// the class-LUT encoder, its pack and the conv weight gradient: every odd window edge 3 .. 63 (view_size 1 .. 31)
static bool encode_edge_ok(int V) { return V >= SSD_ENCODE_EDGE_MIN && V <= SSD_ENCODE_EDGE_MAX && (V & 1); }
#define SSD_EDGE_MSG ": view_edge must be odd, 3 .. 63 (view_size 1 .. 31)"

int ssd_conv_wgrad_codes(const uint8_t* codes, const float* d_conv, float* partial, int32_t rows, int32_t view_edge, void* stream) {
    if (!codes || !d_conv || !partial || rows < 1) return fail(SSD_ERR_INVALID, "bad argument");
    if (!encode_edge_ok(view_edge)) return fail(SSD_ERR_UNSUPPORTED, "ssd_conv_wgrad_codes" SSD_EDGE_MSG);
    if (launch_conv_wgrad(codes, d_conv, partial, rows, view_edge, (hipStream_t)stream)) return fail(SSD_ERR_UNSUPPORTED, "ssd_conv_wgrad_codes" SSD_EDGE_MSG);
    return launched();
}

static int check_encode(const ssd_policy_encode_args* a) {
    if (!a || !a->codes || !a->conv_frags || !a->lin_frags || !a->conv_b || !a->lin_b || a->rows < 1 || a->n_agents < 1 || a->rows % a->n_agents)
        return fail(SSD_ERR_INVALID, "bad argument");
    if (!encode_edge_ok(a->view_edge)) return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_encode" SSD_EDGE_MSG "; use ssd_conv_leaky + GEMM");
    const bool shipped = a->view_edge == 15 || a->view_edge == 31;
    if (!shipped && a->layout != SSD_ENCODE_LAYOUT_LUT)
        return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_encode: the Toeplitz layout is instantiated for 15 x 15 / 31 x 31 windows; other edges take SSD_ENCODE_LAYOUT_LUT");
    if (a->precision != 0 && a->precision != 1 && a->precision != 2) return fail(SSD_ERR_INVALID, "precision must be 1 (bf16) or 2 (f32-equivalent)");
    if (a->alphabet != SSD_CODE_CLASS && a->alphabet != SSD_CODE_CHANNEL_MASK) return fail(SSD_ERR_INVALID, "alphabet");
    if (a->layout != SSD_ENCODE_LAYOUT_TOEPLITZ && a->layout != SSD_ENCODE_LAYOUT_LUT) return fail(SSD_ERR_INVALID, "layout");
    if (a->act && shipped && a->layout != SSD_ENCODE_LAYOUT_TOEPLITZ)
        return fail(SSD_ERR_INVALID, "the activation output (training forward) takes the Toeplitz images at 15 x 15 / 31 x 31");
    const int bands = SSD_ENCODE_BANDS(a->view_edge);
    if (bands == 1 ? (!a->out || a->part || a->out_stride < 32) : (!a->part || a->out)) return fail(SSD_ERR_INVALID, "one band writes `out`, several bands write `part`");
    if ((reinterpret_cast<uintptr_t>(a->conv_frags) | reinterpret_cast<uintptr_t>(a->lin_frags) | reinterpret_cast<uintptr_t>(a->part)) & 15)
        return fail(SSD_ERR_INVALID, "conv_frags / lin_frags / part must be 16-byte aligned");
    const long VV = (long)a->view_edge * a->view_edge;
    if (a->agent_stride < VV || a->env_stride < (long)a->n_agents * a->agent_stride || a->slot_stride < 0 || (a->slot_stride && !a->slot_t))
        return fail(SSD_ERR_INVALID, "env_stride / slot_stride / agent_stride / slot_t");
    if (a->code_bytes < (long)(a->rows / a->n_agents - 1) * a->env_stride + (long)(a->n_agents - 1) * a->agent_stride + VV)
        return fail(SSD_ERR_INVALID, "code_bytes does not cover the rows");
    if (a->slot_t_copy && (!a->slot_t || a->slot_t_copy == a->slot_t)) return fail(SSD_ERR_INVALID, "slot_t_copy needs a distinct slot_t");
    if (a->slot_add < 0 || (a->slot_add && !a->slot_t)) return fail(SSD_ERR_INVALID, "slot_add needs slot_t");
    return SSD_OK;
}

int ssd_policy_encode(const ssd_policy_encode_args* a, void* stream) {
    if (const int bad = check_encode(a)) return bad;
    const int rc = launch_policy_encode(a, (hipStream_t)stream);
    if (rc) return fail(SSD_ERR_DEVICE, "hipFuncSetAttribute(max dynamic LDS) failed");
    return launched();
}

int ssd_policy_pack_encoder_lut(const float* conv_w, const float* conv_b, const float* lin_w, int32_t view_edge, int32_t precision, void* table,
                                void* lin_frags, void* stream) {
    if (!conv_w || !conv_b || !lin_w || !table || !lin_frags) return fail(SSD_ERR_INVALID, "null argument");
    if (precision != 1 && precision != 2) return fail(SSD_ERR_INVALID, "precision must be 1 or 2");
    if ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(lin_frags)) & 15) return fail(SSD_ERR_INVALID, "images must be 16-byte aligned");
    if (!encode_edge_ok(view_edge)) return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_pack_encoder_lut" SSD_EDGE_MSG);
    if (launch_pack_encoder_lut(conv_w, conv_b, lin_w, view_edge, precision, table, lin_frags, (hipStream_t)stream))
        return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_pack_encoder_lut" SSD_EDGE_MSG);
    return launched();
}

int ssd_policy_pack_encoder(const float* conv_w, const float* conv_b, const float* lin_w, int32_t view_edge, int32_t precision, void* conv_frags,
                            void* lin_frags, void* stream) {
    if (!conv_w || !conv_b || !lin_w || !conv_frags || !lin_frags) return fail(SSD_ERR_INVALID, "null argument");
    if (precision != 1 && precision != 2) return fail(SSD_ERR_INVALID, "precision must be 1 or 2");
    if ((reinterpret_cast<uintptr_t>(conv_frags) | reinterpret_cast<uintptr_t>(lin_frags)) & 15) return fail(SSD_ERR_INVALID, "fragment images must be 16-byte aligned");
    if (launch_pack_encoder(conv_w, conv_b, lin_w, view_edge, precision, conv_frags, lin_frags, (hipStream_t)stream))
        return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_pack_encoder: view_edge must be 15 or 31");
    return launched();
}

int ssd_policy_pack_head(const ssd_policy_head_params* p, int32_t precision, void* image, void* stream) {
    if (!p || !image || !p->fc1_w || !p->fc1_b || !p->fc2_w || !p->fc2_b || !p->fc2_v_w || !p->fc2_v_b) return fail(SSD_ERR_INVALID, "null argument");
    for (int g = 0; g < 3; ++g) if (!p->w_i[g] || !p->w_h[g] || !p->b_i[g] || !p->b_h[g]) return fail(SSD_ERR_INVALID, "null GRU parameter");
    if (precision != 1 && precision != 2) return fail(SSD_ERR_INVALID, "precision must be 1 or 2");
    if (p->input_flags & SSD_INPUT_GATHER_ONEHOT) {       // every one-hot block as gathered rows: the dense blocks always fit the image
        const uint32_t fl = p->input_flags;
        if (p->n_actions < 1 || p->n_agents < 1 || p->n_agents > SSD_MAX_AGENTS)
            return fail(SSD_ERR_INVALID, "ssd_policy_pack_head: SSD_INPUT_GATHER_ONEHOT needs n_actions and 1 .. SSD_MAX_AGENTS agents");
        if (fl & ~(SSD_INPUT_EXPLICIT | SSD_INPUT_GATHER_ONEHOT | 127u)) return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_pack_head: input_flags holds a block no head builds");
        const int full = 32 + ((fl & SSD_INPUT_LAST_ACTION) ? p->n_actions : 0) + ((fl & SSD_INPUT_AGENT_ID) ? p->n_agents : 0) +
                         ((fl & SSD_INPUT_REWARD) ? 1 : 0) + ((fl & SSD_INPUT_INC_REWARD) ? 1 : 0) +
                         ((fl & SSD_INPUT_OTHERS_LAST_ACTION) ? p->n_agents * p->n_actions : 0) +
                         ((fl & SSD_INPUT_DISTANCE) ? p->n_agents : 0) + ((fl & SSD_INPUT_AGENT_POS) ? 2 : 0);
        if ((p->fc1_in != full && p->fc1_in != full + p->n_actions) || p->n_actions > 15 || p->fc2_in < 64 || p->fc2_in > 80 || p->fc2_out < 1 || p->fc2_out > 15)
            return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_pack_head: SSD_INPUT_GATHER_ONEHOT: fc1_in = 32 + the widths of the input_flags blocks (inc head: + n_actions), 64 <= fc2_in <= 80, fc2_out <= 15");
        if (!p->onehot_rows || (reinterpret_cast<uintptr_t>(p->onehot_rows) & 15))
            return fail(SSD_ERR_INVALID, "ssd_policy_pack_head: SSD_INPUT_GATHER_ONEHOT needs onehot_rows, 16-byte aligned");
        if (reinterpret_cast<uintptr_t>(image) & 15) return fail(SSD_ERR_INVALID, "image must be 16-byte aligned");
        launch_pack_head(p, precision, image, (hipStream_t)stream);
        return launched();
    }
    const bool others = (p->input_flags & SSD_INPUT_OTHERS_LAST_ACTION) != 0;
    if (others && (p->n_actions < 1 || p->n_agents < 1)) return fail(SSD_ERR_INVALID, "ssd_policy_pack_head: obs_others_last_action needs n_actions");
    const int dense_in = p->fc1_in - (others ? p->n_agents * p->n_actions : 0);
    if (others) {           // the dense rows in front of the block must exist in fc1_w
        const uint32_t fl = p->input_flags;
        const int off = 32 + ((fl & SSD_INPUT_LAST_ACTION) ? p->n_actions : 0) + ((fl & SSD_INPUT_AGENT_ID) ? p->n_agents : 0) +
                        ((fl & SSD_INPUT_REWARD) ? 1 : 0) + ((fl & SSD_INPUT_INC_REWARD) ? 1 : 0);
        if (dense_in < off) return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_pack_head: fc1_in is narrower than the blocks of input_flags");
    }
    if (p->n_agents < 1 || dense_in < 1 || dense_in > 64 || p->fc2_in < 64 || p->fc2_in > 80 || p->fc2_out < 1 || p->fc2_out > 15)
        return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_pack_head: fc1_in (less the others' last-action block) <= 64, 64 <= fc2_in <= 80, fc2_out <= 15");
    if (others && (!p->others_rows || (reinterpret_cast<uintptr_t>(p->others_rows) & 15)))
        return fail(SSD_ERR_INVALID, "ssd_policy_pack_head: obs_others_last_action needs others_rows, 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(image) & 15) return fail(SSD_ERR_INVALID, "image must be 16-byte aligned");
    launch_pack_head(p, precision, image, (hipStream_t)stream);
    return launched();
}

static int check_head(const ssd_policy_head* a, int inc) {
    if (!a || !a->inputs || !a->h || !a->weights || !a->epsilon || !a->step || !a->out_actions) return fail(SSD_ERR_INVALID, "bad argument");
    if (a->n_env < 1 || a->n_agents < 1 || a->n_actions < 1) return fail(SSD_ERR_INVALID, "bad argument");
    if (reinterpret_cast<uintptr_t>(a->epsilon_rows) & 3) return fail(SSD_ERR_INVALID, "ssd_policy_head: epsilon_rows (f32 [n_env]) must be 4-byte aligned");
    if (a->precision != 0 && a->precision != 1 && a->precision != 2) return fail(SSD_ERR_INVALID, "precision must be 1 (bf16) or 2 (f32-equivalent)");
    if (a->feat_part && (inc || a->feat_bands < 1 || !a->lin_b || (reinterpret_cast<uintptr_t>(a->feat_part) & 15)))
        return fail(SSD_ERR_INVALID, "feat_part (env head only) needs feat_bands >= 1, lin_b and 16-byte alignment");
    if (!inc && (a->pos_copy || a->dst_pos) && (!a->orient || (a->pos_copy && !a->orient_copy) || (a->dst_pos && !a->dst_orient)))
        return fail(SSD_ERR_INVALID, "pos_copy / dst_pos need orient and their orient twin");
    const bool files = a->dst_pos || a->dst_actions || a->dst_actions_inc || a->dst_reward || a->next_t_out;
    if (files && (!a->t_index || a->t_slots < 1)) return fail(SSD_ERR_INVALID, "filing into the episode storage needs t_index and t_slots");
    if (a->next_t_out && a->next_t_out == a->t_index) return fail(SSD_ERR_INVALID, "next_t_out must not alias t_index");
    if (a->dst_actions && !a->dst_actions_onehot) return fail(SSD_ERR_INVALID, "dst_actions needs dst_actions_onehot");
    if (a->dst_reward && (!a->dst_clean_num || !a->dst_apple_den)) return fail(SSD_ERR_INVALID, "dst_reward needs dst_clean_num and dst_apple_den");
    if (a->dst_terminated && !a->terminated) return fail(SSD_ERR_INVALID, "dst_terminated needs terminated");
    if (inc ? (!a->actions || !a->pos_pre || !a->orient_pre || !a->reward || !a->clean_num || !a->apple_den)
            : (!a->prev_actions || !a->prev_reward || (!a->prev_actions_inc && !a->recv_inc) || !a->pos)) return fail(SSD_ERR_INVALID, "missing head input");
    if ((a->recv_inc || a->recv_inc_out) && (a->n_agents > 16 || ((reinterpret_cast<uintptr_t>(a->recv_inc) | reinterpret_cast<uintptr_t>(a->recv_inc_out)) & 15)))
        return fail(SSD_ERR_INVALID, "recv_inc / recv_inc_out: 16-byte records (n_agents <= 16), 16-byte aligned");
    if (inc ? (a->recv_inc != nullptr) : (a->recv_inc_out != nullptr)) return fail(SSD_ERR_INVALID, "recv_inc is the env head's input, recv_inc_out the inc head's output");
    // layout limits of the fused kernel: 32 encoder features + tail (+ one-hot action for inc) within 64 columns, 16 fc2 rows
    {
        const uint32_t fl = a->input_flags ? (a->input_flags & ~SSD_INPUT_EXPLICIT) : (uint32_t)SSD_INPUT_FLAGS_SHIPPED;
        if (fl & ~(127u | SSD_INPUT_GATHER_ONEHOT)) return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_head: input_flags holds a block the fused head does not build");
        const bool onehot = (fl & SSD_INPUT_GATHER_ONEHOT) != 0;           // every one-hot block as gathered rows of fc1
        const bool others = !onehot && (fl & SSD_INPUT_OTHERS_LAST_ACTION) != 0;      // gathered rows of fc1, not columns of the image
        const int block = (fl & SSD_INPUT_OTHERS_LAST_ACTION) ? a->n_agents * a->n_actions : 0;
        const int tail = ((fl & SSD_INPUT_LAST_ACTION) ? a->n_actions : 0) + ((fl & SSD_INPUT_AGENT_ID) ? a->n_agents : 0) +
                         ((fl & SSD_INPUT_REWARD) ? 1 : 0) + ((fl & SSD_INPUT_INC_REWARD) ? 1 : 0) +
                         ((fl & SSD_INPUT_DISTANCE) ? a->n_agents : 0) + ((fl & SSD_INPUT_AGENT_POS) ? 2 : 0);
        if (onehot) {       // the dense columns (at most 32 + 1 + 1 + n + 2) always fit: only the width has to match the flags
            if (a->input_shape != 32 + tail + block || a->n_actions + 7 > 16)
                return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_head: SSD_INPUT_GATHER_ONEHOT: input_shape must be 32 + the width of the input_flags blocks");
            if (!a->onehot_rows || !a->prev_record) return fail(SSD_ERR_INVALID, "ssd_policy_head: SSD_INPUT_GATHER_ONEHOT needs onehot_rows and prev_record");
            if (a->n_agents > SSD_MAX_AGENTS) return fail(SSD_ERR_INVALID, "ssd_policy_head: SSD_INPUT_GATHER_ONEHOT takes at most SSD_MAX_AGENTS agents");
            if ((reinterpret_cast<uintptr_t>(a->onehot_rows) | reinterpret_cast<uintptr_t>(a->prev_record) | reinterpret_cast<uintptr_t>(a->prev_record_out)) & 15)
                return fail(SSD_ERR_INVALID, "ssd_policy_head: onehot_rows / prev_record / prev_record_out must be 16-byte aligned");
            if (a->prev_record_out && (inc || a->prev_record_out == a->prev_record))
                return fail(SSD_ERR_INVALID, "ssd_policy_head: prev_record_out is the env head's output and the other buffer of the pair");
        } else if (a->input_shape != 32 + tail + block || 32 + tail + a->n_actions > 64 || a->n_actions + 7 > 16)
            return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_head: input_shape must be 32 + the width of the input_flags blocks and fit 64 columns");
        if (others) {
            if (!a->others_rows || !a->prev_record) return fail(SSD_ERR_INVALID, "ssd_policy_head: obs_others_last_action needs others_rows and prev_record");
            if (a->n_agents > SSD_MAX_AGENTS) return fail(SSD_ERR_INVALID, "ssd_policy_head: obs_others_last_action takes at most SSD_MAX_AGENTS agents");
            if ((reinterpret_cast<uintptr_t>(a->others_rows) | reinterpret_cast<uintptr_t>(a->prev_record) | reinterpret_cast<uintptr_t>(a->prev_record_out)) & 15)
                return fail(SSD_ERR_INVALID, "ssd_policy_head: others_rows / prev_record / prev_record_out must be 16-byte aligned");
            if (a->prev_record_out && (inc || a->prev_record_out == a->prev_record))
                return fail(SSD_ERR_INVALID, "ssd_policy_head: prev_record_out is the env head's output and the other buffer of the pair");
        }
    }
    if ((reinterpret_cast<uintptr_t>(a->inputs) | reinterpret_cast<uintptr_t>(a->h) | reinterpret_cast<uintptr_t>(a->weights)) & 15)
        return fail(SSD_ERR_INVALID, "inputs / h / weights must be 16-byte aligned");
    if (inc ? (a->t_copy_out || a->step_copy_out) : (a->next_step_out != nullptr))
        return fail(SSD_ERR_INVALID, "counter hand-over: the env head writes the copies, the inc head the next values");
    if ((a->next_step_out && a->next_step_out == a->step) || (a->t_copy_out && (!a->t_index || a->t_copy_out == a->t_index)) ||
        (a->step_copy_out && a->step_copy_out == a->step))
        return fail(SSD_ERR_INVALID, "counter hand-over: a launch must not write a scalar it reads");
    return SSD_OK;
}

static int policy_head(const ssd_policy_head* a, int inc, void* stream) {
    if (const int bad = check_head(a, inc)) return bad;
    const int rc = launch_policy_head(a, inc, (hipStream_t)stream);
    if (rc == -3) return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_head is instantiated for n_actions 9 (Cleanup) and 8 (Harvest)");
    if (rc) return fail(SSD_ERR_DEVICE, "ssd_policy_head: launch / hipFuncSetAttribute(max dynamic LDS) failed");
    return launched();
}
// the same launch for the gathered head layouts (k_inc_encode_gather): ssd_policy_head.pipeline_gather asks for it
static int policy_head_inc_encode_gather(const ssd_policy_head* h, const ssd_policy_encode_args* e, void* stream) {
    if (!e) return fail(SSD_ERR_INVALID, "bad argument");
    if (!h->input_flags || !(h->input_flags & (SSD_INPUT_OTHERS_LAST_ACTION | SSD_INPUT_GATHER_ONEHOT)))
        return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_head_inc_encode: pipeline_gather is for SSD_INPUT_OTHERS_LAST_ACTION / SSD_INPUT_GATHER_ONEHOT heads; every other input set leaves it zero");
    if (const int bad = check_head(h, 1)) return bad;
    if (!encode_edge_ok(e->view_edge)) return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_head_inc_encode (pipeline_gather)" SSD_EDGE_MSG);
    if (e->layout == SSD_ENCODE_LAYOUT_TOEPLITZ)
        return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_head_inc_encode: pipeline_gather takes SSD_ENCODE_LAYOUT_LUT at every edge (the Toeplitz layout: ssd_policy_encode + ssd_policy_head_inc)");
    if (const int bad = check_encode(e)) return bad;
    if (e->act || e->slot_t_copy || e->counter_inc) return fail(SSD_ERR_INVALID, "ssd_policy_head_inc_encode: no act / slot_t_copy / counter_inc");
    if ((h->precision == 1) != (e->precision == 1)) return fail(SSD_ERR_INVALID, "ssd_policy_head_inc_encode: one precision for both halves");
    if (e->out == h->inputs) return fail(SSD_ERR_INVALID, "ssd_policy_head_inc_encode: the encoder must write the other inputs buffer");
    if (e->slot_t && (e->slot_t == h->next_t_out))
        return fail(SSD_ERR_INVALID, "ssd_policy_head_inc_encode: the encoder must not read the scalar the inc head writes");
    if (h->n_actions != 9 && h->n_actions != 8)
        return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_head_inc_encode (pipeline_gather) is instantiated for n_actions 9 (Cleanup) and 8 (Harvest)");
    const int rc = launch_policy_inc_encode_gather(h, e, (hipStream_t)stream);
    if (rc == -3 || rc == -2) return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_head_inc_encode (pipeline_gather): no instance for this action count / edge / layout");
    if (rc) return fail(SSD_ERR_DEVICE, "ssd_policy_head_inc_encode: launch / hipFuncSetAttribute(max dynamic LDS) failed");
    return launched();
}
int ssd_policy_head_inc_encode(const ssd_policy_head* h, const ssd_policy_encode_args* e, void* stream) {
    if (h && h->pipeline_gather) return policy_head_inc_encode_gather(h, e, stream);
    if (h && h->input_flags && (h->input_flags & SSD_INPUT_GATHER_ONEHOT))
        return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_head_inc_encode: SSD_INPUT_GATHER_ONEHOT takes ssd_policy_encode + ssd_policy_head_inc");
    if (h && h->input_flags && (h->input_flags & SSD_INPUT_OTHERS_LAST_ACTION))
        return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_head_inc_encode: obs_others_last_action takes ssd_policy_encode + ssd_policy_head_inc");
    if (const int bad = check_head(h, 1)) return bad;
    if (const int bad = check_encode(e)) return bad;
    if (e->act || e->slot_t_copy || e->counter_inc) return fail(SSD_ERR_INVALID, "ssd_policy_head_inc_encode: no act / slot_t_copy / counter_inc");
    if ((h->precision == 1) != (e->precision == 1)) return fail(SSD_ERR_INVALID, "ssd_policy_head_inc_encode: one precision for both halves");
    if (e->out == h->inputs) return fail(SSD_ERR_INVALID, "ssd_policy_head_inc_encode: the encoder must write the other inputs buffer");
    if (e->slot_t && (e->slot_t == h->next_t_out)) return fail(SSD_ERR_INVALID, "ssd_policy_head_inc_encode: the encoder must not read the scalar the inc head writes");
    const int rc = launch_policy_inc_encode(h, e, (hipStream_t)stream);
    if (rc == -3) return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_head is instantiated for n_actions 9 (Cleanup) and 8 (Harvest)");
    if (rc == -2) return fail(SSD_ERR_UNSUPPORTED, "ssd_policy_head_inc_encode takes the Toeplitz layout at 15 x 15 / 31 x 31 windows only; every other odd edge 3 .. 63 takes SSD_ENCODE_LAYOUT_LUT (or ssd_policy_encode + ssd_policy_head_inc)");
    if (rc) return fail(SSD_ERR_DEVICE, "ssd_policy_head_inc_encode: launch / hipFuncSetAttribute(max dynamic LDS) failed");
    return launched();
}
int ssd_policy_head_plan(int32_t n_env, int32_t n_agents, int32_t fused_with_encoder, int32_t* workgroups_per_agent, int32_t* compute_waves,
                         int32_t* tiles_per_wave) {
    if (!workgroups_per_agent || !compute_waves || !tiles_per_wave) return fail(SSD_ERR_INVALID, "null argument");
    if (n_env < 1 || n_agents < 1) return fail(SSD_ERR_INVALID, "ssd_policy_head_plan: n_env, n_agents >= 1");
    if (fused_with_encoder < 0 || fused_with_encoder > 2)
        return fail(SSD_ERR_INVALID, "ssd_policy_head_plan: the third argument is 0 (standalone dense heads), 1 (fused with the encoder) or 2 (standalone gathered heads)");
    int a = 0, b = 0, c = 0;
    policy_head_plan(n_env, n_agents, fused_with_encoder, &a, &b, &c);
    *workgroups_per_agent = a; *compute_waves = b; *tiles_per_wave = c;
    return SSD_OK;
}
int ssd_policy_head_env(const ssd_policy_head* a, void* stream) { return policy_head(a, 0, stream); }
int ssd_policy_head_inc(const ssd_policy_head* a, void* stream) { return policy_head(a, 1, stream); }

}  // extern "C"
