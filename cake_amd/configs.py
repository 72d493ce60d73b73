"""BASELINE.json model configurations (architecture shapes only; weights are
random-init — no network for checkpoints).  Shapes per SURVEY.md §8 header."""

LLAMA3_8B = dict(
    model_type="llama", hidden_size=4096, intermediate_size=14336,
    vocab_size=128256, num_hidden_layers=32, num_attention_heads=32,
    num_key_value_heads=8, head_dim=128, rms_norm_eps=1e-5,
    rope_theta=500000.0, max_position_embeddings=8192,
    tie_word_embeddings=False,
    rope_scaling=dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0,
                      high_freq_factor=4.0,
                      original_max_position_embeddings=8192))

LLAMA3_70B = dict(
    model_type="llama", hidden_size=8192, intermediate_size=28672,
    vocab_size=128256, num_hidden_layers=80, num_attention_heads=64,
    num_key_value_heads=8, head_dim=128, rms_norm_eps=1e-5,
    rope_theta=500000.0, max_position_embeddings=8192,
    tie_word_embeddings=False,
    rope_scaling=dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0,
                      high_freq_factor=4.0,
                      original_max_position_embeddings=8192))

QWEN3_0_6B = dict(
    model_type="qwen3", hidden_size=1024, intermediate_size=3072,
    vocab_size=151936, num_hidden_layers=28, num_attention_heads=16,
    num_key_value_heads=8, head_dim=128, rms_norm_eps=1e-6,
    rope_theta=1000000.0, max_position_embeddings=8192,
    tie_word_embeddings=True)

QWEN3_32B = dict(
    model_type="qwen3", hidden_size=5120, intermediate_size=25600,
    vocab_size=151936, num_hidden_layers=64, num_attention_heads=64,
    num_key_value_heads=8, head_dim=128, rms_norm_eps=1e-6,
    rope_theta=1000000.0, max_position_embeddings=8192,
    tie_word_embeddings=False)

QWEN3_32B_FP8 = dict(QWEN3_32B,
    quantization_config=dict(quant_method="fp8",
                             weight_block_size=[128, 128]))

# Mistral-7B-v0.1 shape (mistral/, 196 LoC of the same common Transformer +
# the sliding-window flag cache.rs:173-205 consumes; window now runs in the
# attention kernels' span bound)
MISTRAL_7B = dict(
    model_type="mistral", hidden_size=4096, intermediate_size=14336,
    vocab_size=32000, num_hidden_layers=32, num_attention_heads=32,
    num_key_value_heads=8, head_dim=128, rms_norm_eps=1e-5,
    rope_theta=10000.0, max_position_embeddings=32768,
    tie_word_embeddings=False, sliding_window=4096,
)

# Llama-3-8B with AutoGPTQ 4-bit weights (group 128, no act-order): the seven
# projections of every layer are 4-bit, embedding / lm_head / norms 16-bit
LLAMA3_8B_GPTQ = dict(LLAMA3_8B,
    quantization_config=dict(quant_method="gptq", bits=4, group_size=128,
                             desc_act=False, sym=True))

# Qwen2.5 (qwen2/): the llama-shaped Transformer plus an additive bias on the
# q, k and v projections (qwen2/config.rs:84).  The official GPTQ-Int4
# checkpoints are group 128 without act-order and keep F16 biases.
QWEN2_5_0_5B = dict(
    model_type="qwen2", hidden_size=896, intermediate_size=4864,
    vocab_size=151936, num_hidden_layers=24, num_attention_heads=14,
    num_key_value_heads=2, head_dim=64, rms_norm_eps=1e-6,
    rope_theta=1000000.0, max_position_embeddings=32768,
    tie_word_embeddings=True)

QWEN2_5_7B = dict(
    model_type="qwen2", hidden_size=3584, intermediate_size=18944,
    vocab_size=152064, num_hidden_layers=28, num_attention_heads=28,
    num_key_value_heads=4, head_dim=128, rms_norm_eps=1e-6,
    rope_theta=1000000.0, max_position_embeddings=32768,
    tie_word_embeddings=False)

QWEN2_5_7B_GPTQ = dict(QWEN2_5_7B,
    quantization_config=dict(quant_method="gptq", bits=4, group_size=128,
                             desc_act=False, sym=True))

# Phi-4 family (phi4/, HF model_type "phi3"): llama-shaped, but the checkpoint
# ships self_attn.qkv_proj and mlp.gate_up_proj fused (phi4/config.rs:88-89).
# Phi-4-mini also rotates only the first 96 of 128 head dims and scales its
# frequencies by LongRoPE.
PHI_4 = dict(
    model_type="phi3", hidden_size=5120, intermediate_size=17920,
    vocab_size=100352, num_hidden_layers=40, num_attention_heads=40,
    num_key_value_heads=10, rms_norm_eps=1e-5, rope_theta=250000.0,
    max_position_embeddings=16384, tie_word_embeddings=False)

# The published 48-entry short_factor / long_factor lists are not reproduced
# here: these are monotone PLACEHOLDERS of the right length (short 1.0 .. 1.5,
# long 1.0 .. 30).  They set table values only and do not affect speed; a real
# run takes the lists from the checkpoint's config.json.
PHI_4_MINI = dict(
    model_type="phi3", hidden_size=3072, intermediate_size=8192,
    vocab_size=200064, num_hidden_layers=32, num_attention_heads=24,
    num_key_value_heads=8, head_dim=128, rms_norm_eps=1e-5,
    rope_theta=10000.0, partial_rotary_factor=0.75,
    max_position_embeddings=131072, original_max_position_embeddings=4096,
    tie_word_embeddings=True,
    rope_scaling=dict(
        type="longrope",
        short_factor=[1.0 + 0.5 * i / 47 for i in range(48)],
        long_factor=[1.0 + 29.0 * i / 47 for i in range(48)]))

PHI_4_GPTQ = dict(PHI_4,
    quantization_config=dict(quant_method="gptq", bits=4, group_size=128,
                             desc_act=False, sym=True))

# Falcon3 (falcon3/, HF model_type "llama"): a plain llama-shaped model with
# 256-wide heads and four kv heads (G = 2 in 1B, 3 in the others).  Shapes as
# published, written down from memory: nothing here could check them against
# the checkpoints' config.json, which a real run reads anyway.
_FALCON3 = dict(
    model_type="llama", head_dim=256, num_key_value_heads=4,
    vocab_size=131072, rms_norm_eps=1e-6, rope_theta=1000042.0,
    max_position_embeddings=32768, tie_word_embeddings=False)

FALCON3_1B = dict(_FALCON3, hidden_size=2048, intermediate_size=8192,
                  num_hidden_layers=18, num_attention_heads=8)
FALCON3_3B = dict(_FALCON3, hidden_size=3072, intermediate_size=9216,
                  num_hidden_layers=22, num_attention_heads=12)
FALCON3_7B = dict(_FALCON3, hidden_size=3072, intermediate_size=23040,
                  num_hidden_layers=28, num_attention_heads=12)
FALCON3_10B = dict(FALCON3_7B, num_hidden_layers=40)

# Gemma 3 text models (gemma3/, HF model_type "gemma3_text"): four (1 + w)
# norms per layer, QK-norm, GELU-tanh gate, scaled embedding, tied head, five
# local (sliding-window, rope base 1e4) layers to one global (rope base 1e6,
# linear factor 8 from 4B up).  Shapes as published, written down from memory
# like Falcon3's: no config file was at hand to check them against, and a real
# run reads the checkpoint's config.json anyway.
_GEMMA3 = dict(
    model_type="gemma3_text", head_dim=256, vocab_size=262208,
    rms_norm_eps=1e-6, rope_theta=1000000.0, rope_local_base_freq=10000.0,
    sliding_window=1024, sliding_window_pattern=6, query_pre_attn_scalar=256,
    hidden_activation="gelu_pytorch_tanh", max_position_embeddings=131072,
    rope_scaling=dict(rope_type="linear", factor=8.0),
    tie_word_embeddings=True)

GEMMA3_1B = dict(_GEMMA3, hidden_size=1152, intermediate_size=6912,
                 num_hidden_layers=26, num_attention_heads=4,
                 num_key_value_heads=1, vocab_size=262144,
                 sliding_window=512, max_position_embeddings=32768,
                 rope_scaling=None)
GEMMA3_4B = dict(_GEMMA3, hidden_size=2560, intermediate_size=10240,
                 num_hidden_layers=34, num_attention_heads=8,
                 num_key_value_heads=4)
GEMMA3_12B = dict(_GEMMA3, hidden_size=3840, intermediate_size=15360,
                  num_hidden_layers=48, num_attention_heads=16,
                  num_key_value_heads=8)
GEMMA3_27B = dict(_GEMMA3, hidden_size=5376, intermediate_size=21504,
                  num_hidden_layers=62, num_attention_heads=32,
                  num_key_value_heads=16, head_dim=128,
                  query_pre_attn_scalar=168)

MODELS = {
    "llama3-8b": LLAMA3_8B,
    "llama3-70b": LLAMA3_70B,
    "qwen3-0.6b": QWEN3_0_6B,
    "mistral-7b": MISTRAL_7B,
    "qwen3-32b": QWEN3_32B,
    "qwen3-32b-fp8": QWEN3_32B_FP8,
}


# quantized variants live beside MODELS (the pinned bf16/fp8 table)
QUANT_MODELS = {
    "llama3-8b-gptq": LLAMA3_8B_GPTQ,
}


# the qwen2 family (q/k/v projection bias), beside the two tables above
QWEN2_MODELS = {
    "qwen2.5-0.5b": QWEN2_5_0_5B,
    "qwen2.5-7b": QWEN2_5_7B,
    "qwen2.5-7b-gptq": QWEN2_5_7B_GPTQ,
}


# the phi3 family (fused checkpoint tensors; partial rotary and LongRoPE in
# phi-4-mini)
PHI_MODELS = {
    "phi-4": PHI_4,
    "phi-4-mini": PHI_4_MINI,
    "phi-4-gptq": PHI_4_GPTQ,
}


# the falcon3 family (head_dim 256)
FALCON3_MODELS = {
    "falcon3-1b": FALCON3_1B,
    "falcon3-3b": FALCON3_3B,
    "falcon3-7b": FALCON3_7B,
    "falcon3-10b": FALCON3_10B,
}


# the gemma3 family (sandwich norms, GELU gate, local and global layers)
GEMMA3_MODELS = {
    "gemma-3-1b": GEMMA3_1B,
    "gemma-3-4b": GEMMA3_4B,
    "gemma-3-12b": GEMMA3_12B,
    "gemma-3-27b": GEMMA3_27B,
}


def find_model(name: str) -> dict:
    """The config called `name` in MODELS, QUANT_MODELS, QWEN2_MODELS,
    PHI_MODELS, FALCON3_MODELS or GEMMA3_MODELS."""
    for table in (MODELS, QUANT_MODELS, QWEN2_MODELS, PHI_MODELS,
                  FALCON3_MODELS, GEMMA3_MODELS):
        if name in table:
            return table[name]
    raise KeyError(name)


def weight_bytes(cfg: dict, lo=0, hi=None, embed=True, head=True) -> int:
    """Bytes of weights resident in HBM for this config: bf16, or for a gptq
    config the device 4-bit layout (packed nibbles + an f32 {scale, zero
    term} pair per row and group) with 16-bit embedding, head and norms.  A
    qwen2 config adds its fused f32 q|k|v bias row per layer, a gemma3 config
    (never quantized) its four norm rows and q/k norm rows per layer."""
    if cfg.get("model_type") in ("gemma3_text", "gemma3"):
        return weight_bytes_bf16(cfg, lo, hi, embed, head)
    q = cfg.get("quantization_config") or {}
    H, I, V = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
    nh, nkv = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    hd = cfg.get("head_dim") or H // nh
    L = (hi if hi is not None else cfg["num_hidden_layers"]) - lo
    bias = L * (nh + 2 * nkv) * hd * 4 if cfg.get("model_type") == "qwen2" \
        else 0
    if q.get("quant_method") != "gptq":
        return weight_bytes_bf16(cfg, lo, hi, embed, head) + bias
    g = q.get("group_size", 128)

    def w4(n, k):
        return n * k // 2 + n * (k // (k if g == -1 else g)) * 8
    per_layer = (w4((nh + 2 * nkv) * hd, H) + w4(H, nh * hd) +
                 w4(2 * I, H) + w4(H, I) + 2 * H * 2)
    total = L * per_layer + bias
    if embed:
        total += V * H * 2
    if head:
        total += H * 2
        if not cfg.get("tie_word_embeddings"):
            total += V * H * 2
    return total


def weight_bytes_bf16(cfg: dict, lo=0, hi=None, embed=True, head=True) -> int:
    gemma3 = cfg.get("model_type") in ("gemma3_text", "gemma3")
    if cfg.get("model_type") == "gemma3":    # the text model, HF's defaults
        cfg = {"hidden_size": 2304, "intermediate_size": 9216,
               "vocab_size": 262208, "num_hidden_layers": 26,
               "num_attention_heads": 8, "num_key_value_heads": 4,
               "head_dim": 256, **(cfg.get("text_config") or {})}
    H, I, V = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
    nh, nkv = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    hd = cfg.get("head_dim") or H // nh
    L = (hi if hi is not None else cfg["num_hidden_layers"]) - lo
    per_layer = (nh + 2 * nkv) * hd * H + H * nh * hd + 3 * I * H + 2 * H
    if gemma3:                               # two more norm rows, q/k norm
        per_layer += 2 * H + 2 * hd
    total = L * per_layer
    if embed:
        total += V * H
    if head:
        total += H
        if not (gemma3 or cfg.get("tie_word_embeddings")):
            total += V * H
    return total * 2
