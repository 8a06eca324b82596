// options.cpp -- the kernel-form switches of a net (NetOptions in net.h, where every member carries its default and the measurements behind it) as ONE
// table: a row per option with its key, the environment variable that seeds it when a net is created, the kind of value and the member it sets.
// moe_net_set_option and the MOE_* seeding walk the same rows; a value is parsed into a local and stored only when the row accepts it.
#include "net.h"

using namespace moe;

namespace {

enum OptionKind {
    kFlag,       // 0 | off | 1 | on
    kWords,      // one of the row's words, each storing its number
    kCount,      // a non-negative integer (atoi: a word or the empty string reads as 0)
    kInt,        // whatever atoi makes of it
    kText,       // any string
    kRepeat,     // "<layer key substring>:<n>", n >= 1; "" or "0" clears
};
struct OptionWord { const char* word; int value; };
struct OptionRow {
    const char* key;
    const char* env;                      // nullptr: set through moe_net_set_option only
    OptionKind kind;
    int NetOptions::*num;                 // every kind but kText / kRepeat
    std::string NetOptions::*text;        // kText
    OptionWord words[3];                  // kWords
};
constexpr OptionWord kOnOff[] = {{"0", 0}, {"off", 0}, {"1", 1}, {"on", 1}};

const OptionRow kOptionTable[] = {
    {"conv_impl", "MOE_CONV_IMPL", kWords, &NetOptions::conv_impl, nullptr, {{"sp", 2}, {"v1", 0}}},
    {"sp_impl", "MOE_SP_IMPL", kWords, &NetOptions::sp_impl, nullptr, {{"sp", 0}, {"auto", 1}, {"rw", 2}}},
    {"tail_split", "MOE_TAIL_SPLIT", kWords, &NetOptions::tail_split, nullptr, {{"0", 0}, {"r", 1}, {"ru", 2}}},
    {"tail_form", "MOE_TAIL_FORM", kWords, &NetOptions::tail_form, nullptr, {{"planes", 0}, {"sums", 1}}},
    {"up_impl", "MOE_UP_IMPL", kWords, &NetOptions::up_impl, nullptr, {{"rw", 0}, {"ps4", 1}}},
    {"up_fuse2", "MOE_UP_FUSE2", kFlag, &NetOptions::up_fuse2},
    {"conv1x1", "MOE_CONV1X1", kFlag, &NetOptions::conv1x1},
    {"q8_impl", "MOE_Q8_IMPL", kWords, &NetOptions::q8_impl, nullptr, {{"s", 1}, {"p", 0}}},
    {"exact_fuse", "MOE_EXACT_FUSE", kFlag, &NetOptions::exact_fuse},
    {"branch_streams", "MOE_BRANCH_STREAMS", kFlag, &NetOptions::branch_streams},
    {"branch_groups", "MOE_BRANCH_GROUPS", kCount, &NetOptions::branch_groups},
    {"auto_calibrate", "MOE_AUTO_CALIBRATE", kFlag, &NetOptions::auto_calibrate},
    {"overlap_calls", "MOE_OVERLAP_CALLS", kFlag, &NetOptions::overlap_calls},
    {"overlap_groups", "MOE_OVERLAP_GROUPS", kCount, &NetOptions::overlap_groups},
    {"overlap_fork", "MOE_OVERLAP_FORK", kFlag, &NetOptions::overlap_fork},
    {"s64", "MOE_S64", kFlag, &NetOptions::s64},
    {"k48", "MOE_K48", kFlag, &NetOptions::k48},
    {"x3_impl", "MOE_X3_IMPL", kWords, &NetOptions::x3_impl, nullptr, {{"auto", 0}, {"x3", 1}, {"q8", 2}}},
    {"lo8", "MOE_LO8", kFlag, &NetOptions::lo8},
    {"x3_fuse", "MOE_X3_FUSE", kFlag, &NetOptions::x3_fuse},
    {"arsb_fuse", "MOE_ARSB_FUSE", kFlag, &NetOptions::arsb_fuse},
    {"fuse_tail", "MOE_FUSE_TAIL", kFlag, &NetOptions::fuse_tail},
    {"sedn_fuse", "MOE_SEDN_FUSE", kFlag, &NetOptions::sedn_fuse},
    {"pool_fuse", "MOE_POOL_FUSE", kFlag, &NetOptions::pool_fuse},
    {"frm_pre", "MOE_FRM_PRE", kFlag, &NetOptions::frm_pre},
    {"stem2", "MOE_STEM2", kFlag, &NetOptions::stem2},
    {"lite_lut", "MOE_LITE_LUT", kFlag, &NetOptions::lite_lut},
    {"dbg", "MOE_DBG", kInt, &NetOptions::dbg},
    {"trace_key", "MOE_TRACE_KEY", kText, nullptr, &NetOptions::trace_key},
    {"tiles_per_batch", "MOE_TILES_PER_BATCH", kCount, &NetOptions::tiles_per_batch},
    {"max_groups", "MOE_MAX_GROUPS", kCount, &NetOptions::max_groups},
    {"calib_log", nullptr, kFlag, &NetOptions::calib_log},
    {"repeat", nullptr, kRepeat},
};

bool word_value(const OptionWord* words, size_t n, const char* v, int& out)
{
    for (size_t i = 0; i < n; ++i)
        if (words[i].word && !strcmp(v, words[i].word)) { out = words[i].value; return true; }
    return false;
}

}  // namespace

bool NetOptions::set(const std::string& key, const char* v)
{
    if (!v) return false;
    for (const OptionRow& r : kOptionTable) {
        if (key != r.key) continue;
        int t = 0;
        switch (r.kind) {
            case kFlag: if (!word_value(kOnOff, 4, v, t)) return false; break;
            case kWords: if (!word_value(r.words, 3, v, t)) return false; break;
            case kCount: if ((t = atoi(v)) < 0) return false; break;
            case kInt: t = atoi(v); break;
            case kText: this->*r.text = v; return true;
            case kRepeat: {
                // parsed into locals first: a refused value ("up1:0", "k:-3", "nonsense") must leave the option as it was -- a stored count of zero would issue no launch at all
                // for the matching layers
                const char* c = strrchr(v, ':');
                if (!c) {
                    if (*v && strcmp(v, "0")) return false;
                    repeat_key.clear(); repeat_n = 1;
                    return true;
                }
                const int cnt = atoi(c + 1);
                if (cnt < 1 || c == v) return false;
                repeat_key.assign(v, c - v); repeat_n = cnt;
                return true;
            }
        }
        this->*r.num = t;
        return true;
    }
    return false;
}

void NetOptions::from_env()
{
    for (const OptionRow& r : kOptionTable)
        if (const char* e = r.env ? getenv(r.env) : nullptr)
            if (!set(r.key, e)) fprintf(stderr, "moephoto_amd: %s=\"%s\" is not a value of option %s -- ignored\n", r.env, e, r.key);      // (a typo in an A/B run must not pass silently)

    if (const char* e = getenv("MOE_EXACT_BLOCKS")) exact_blocks_env = atoi(e);
    arsb_trace = getenv("MOE_ARSB_TRACE") != nullptr;
}

extern "C" int moe_net_set_option(moe_net* n, const char* key, const char* value)
{
    if (!n || !key || !value) return fail(MOE_EINVAL, "moe_net_set_option: NULL argument");
    if (!n->opt.set(key, value)) return fail(MOE_EINVAL, "moe_net_set_option: unknown option or value \"%s\" = \"%s\"", key, value);
    drop_lut(*n);      // (a kernel-form switch may change the U branch's bits: the table is refilled by the next fp16 forward)
    if (!strcmp(key, "max_groups") && n->finalized) n->max_groups = n->opt.max_groups > 0 ? n->opt.max_groups : conv_mfma_max_groups();
    return MOE_OK;
}
