// The model handle of libmewzoom_hip.so (mz_host.cpp; mz_debug.cpp reads its dimensions and its schedule): the layers with their
// weights, the registry of parameters, and what its launches share.
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "mz_runner.h"
#include "mz_schedule.h"

enum SlotKind { SK_CONV, SK_ALPHA, SK_STEM_W, SK_STEM_B, SK_QA_B };
// One parameter of the reference's state_dict: its name and shape (mz_weight_info), where its value goes, whether it has been set
struct Slot {
    std::string name;
    int kind;
    mz::ConvW* conv = nullptr;  // SK_CONV: the layer packed from it
    mz::ConvW* also = nullptr;  // ... and a second one: the fused gate (mixf) of a block's skip.conv.weight
    float* alpha = nullptr;     // SK_ALPHA
    bool set = false;
    int64_t shape[4] = {0, 0, 0, 0};
    int ndim = 0;
};

struct mz_handle {
    mz_config cfg;
    mz::ModelDims dims;  // dtype, channels per level, hidden ratio, head levels, quality features
    mz::Model<mz::ConvW> model;  // every layer, planned, with its weights
    mz::DevBuf stem_w4;  // float [cp0][4]
    mz::DevBuf qa_bias;  // float [F]
    std::vector<Slot> slots;
    std::unordered_map<std::string, int> slot_index;
    mz::LaunchCtx ctx;
};
