"""``LlamaModel`` — Python mirror of the reference's model::LlamaModel (include/model/model.h:59-89)
over the fused, graph-captured HIP decode step of libsli.so (engine.hip).

Differences from the reference, all deliberate and documented in DESIGN.md:
  * the model shape is a runtime ``LlamaModelConfig`` (the reference hard-codes config.h:5-17 and
    copies it back in read_model_file, model.cpp:219-230);
  * ``predict`` takes token ids, or text when a ``tokenizer_path`` is given (``encode.SPELayer`` over the Python
    sentencepiece package, encode.cpp:5-27; loaded in ``init`` as create_nonparam_layers does, model.cpp:328);
  * weights are either the reference's flat fp32 file (model_path) or seeded synthetic weights.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, replace

import numpy as np

from . import _lib
from ._lib import CREATE_MX_BATCH, DT_F8E4M3, DT_F16, DT_F32, DT_I8, DT_MXFP4, ModelConfig, call

_DTYPES = {"f32": DT_F32, "fp32": DT_F32, "f16": DT_F16, "fp16": DT_F16, "i8": DT_I8, "int8": DT_I8,
           "mxfp4": DT_MXFP4, "fp4": DT_MXFP4,
           "f8": DT_F8E4M3, "fp8": DT_F8E4M3, "e4m3": DT_F8E4M3}  # K/V cache only (OCP FP8 E4M3, sli.h)
_PREFILL_MODES = {"auto": 0, "gemm": 1, "decode": 2, "gemm-kv8": 3}  # SLI_PREFILL_*


@dataclass(frozen=True)
class LlamaModelConfig:
    """include/model/config.h:5-17 (same field names)."""
    vocab_size: int = 128256
    head_dim: int = 128
    hidden_size: int = 3072
    kv_hidden_size: int = 1024
    intermediate_size: int = 8192
    max_length: int = 1024
    num_hidden_layers: int = 28
    num_attention_heads: int = 24
    num_key_value_heads: int = 8
    rms_norm_eps: float = 1e-5
    rope_theta: float = 100000.0


PRESETS = {
    # BASELINE.json configs[0]: tiny-llama shape (2 layers, d=256, 4 heads), greedy 32 tokens
    "tiny": LlamaModelConfig(512, 64, 256, 256, 768, 64, 2, 4, 4, 1e-5, 10000.0),
    "tiny-gqa": LlamaModelConfig(512, 64, 256, 128, 768, 64, 2, 4, 2, 1e-5, 10000.0),
    # tiny shapes wide enough for tensor parallelism over 8 ranks (heads and kv heads divisible by 8)
    "tiny-h8": LlamaModelConfig(512, 64, 512, 512, 1024, 64, 2, 8, 8, 1e-5, 10000.0),
    "tiny-gqa-h16": LlamaModelConfig(512, 64, 1024, 512, 2048, 64, 2, 16, 8, 1e-5, 10000.0),
    # small head_dim-128 shapes for the persistent layer stack (tp_layers.h: head_dim 128, per-CU shares that fit)
    "small-h128": LlamaModelConfig(1000, 128, 1024, 1024, 2816, 512, 2, 8, 8, 1e-5, 10000.0),
    "small-h128-gqa": LlamaModelConfig(1000, 128, 1024, 512, 2816, 512, 2, 8, 4, 1e-5, 10000.0),
    # configs[1..3]: Llama-2 7B (public model card shape), ctx 2048
    "llama2-7b": LlamaModelConfig(32000, 128, 4096, 4096, 11008, 2048, 32, 32, 32, 1e-5, 10000.0),
    # configs[4]: Llama-3 8B (GQA), ctx 4096
    "llama3-8b": LlamaModelConfig(128256, 128, 4096, 1024, 14336, 4096, 32, 32, 8, 1e-5, 500000.0),
    # the reference's own hard-coded default (config.h:5-17, Llama-3.2-3B shape)
    "reference-default": LlamaModelConfig(),
}


def preset(name: str, **overrides) -> LlamaModelConfig:
    return replace(PRESETS[name], **overrides)


class LlamaModel:
    def __init__(self, tokenizer_path: str = "", model_path: str = "", device_type: str = "cuda",
                 config: LlamaModelConfig | None = None, w_dtype: str = "f16", kv_dtype: str = "f16",
                 act_mode: int = 0, tp_rank: int = 0, tp_size: int = 1, comm_id: bytes | None = None,
                 device: int = 0, seed: int | None = None, batch: int = 1, mx_batch: bool = False):
        if device_type not in ("cuda", "hip"):
            raise ValueError("Device Type ERROR!")  # op/*.cpp dispatch: only the HIP backend exists here
        self.tokenizer_path = tokenizer_path
        self.model_path = model_path
        self.config = config or LlamaModelConfig()
        self.w_dtype = _DTYPES[w_dtype]
        self.kv_dtype = _DTYPES[kv_dtype]
        self.act_mode = act_mode
        self.tp_rank, self.tp_size = tp_rank, tp_size
        self.comm_id = comm_id
        self.device = device
        self.seed = seed
        self.batch = batch  # sequences decoding in lockstep (extension: the reference is batch 1)
        # opt in to MXFP4 weights at batch > 1 (SLI_CREATE_MX_BATCH); no effect on the other weight types
        self.mx_batch = bool(mx_batch)
        self._h = None
        self.encode_layer = None

    # ------------------------------------------------------------------ model.h:63-67
    def _config_struct(self) -> ModelConfig:
        c = self.config
        if c.kv_hidden_size != c.num_key_value_heads * c.head_dim:
            raise ValueError("kv_hidden_size must equal num_key_value_heads * head_dim")
        return ModelConfig(c.vocab_size, c.hidden_size, c.num_attention_heads, c.num_key_value_heads, c.head_dim,
                           c.intermediate_size, c.num_hidden_layers, c.max_length, c.rms_norm_eps, c.rope_theta,
                           self.w_dtype, self.kv_dtype, self.act_mode, self.tp_rank, self.tp_size, self.device,
                           self.batch)

    def init(self) -> "LlamaModel":
        if self.tokenizer_path:  # model.cpp:328 (RuntimeError when the model file does not load, encode.cpp:8-10)
            from .encode import SPELayer
            self.encode_layer = SPELayer(self.tokenizer_path)
        mc = self._config_struct()
        h = ctypes.c_void_p()
        cid = ctypes.create_string_buffer(self.comm_id, len(self.comm_id)) if self.comm_id else None
        if self.mx_batch:
            call("sli_model_create_flags", ctypes.byref(mc), cid, CREATE_MX_BATCH, ctypes.byref(h))
        else:
            call("sli_model_create", ctypes.byref(mc), cid, ctypes.byref(h))
        self._h = h
        return self._load_weights()

    def _load_weights(self) -> "LlamaModel":
        if self.model_path:
            call("sli_model_load_flat", self._h, self.model_path.encode())
        elif self.seed is not None:
            call("sli_model_init_synthetic", self._h, self.seed)
        else:
            raise ValueError("No model weigth file!")  # model.cpp:205-207
        return self

    _borrowed = False  # a rank of a TPGroup: the group owns (steps, destroys) the engine

    def close(self):
        if self._h is not None and not self._borrowed:
            _lib.load().sli_model_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ weights / state
    def set_weight(self, kind: int, index: int, tensor: np.ndarray):
        t = np.ascontiguousarray(tensor, np.float32)
        call("sli_model_set_weight", self._h, kind, index, t.ctypes.data_as(ctypes.c_void_p), t.size)

    def reset(self):
        call("sli_model_reset", self._h)

    def fill_kv_synthetic(self, seed: int, upto: int):
        call("sli_model_fill_kv_synthetic", self._h, seed, upto)

    def set_state(self, token: int, pos: int, advance: bool = True):
        call("sli_model_set_state", self._h, token, pos, 1 if advance else 0)

    def set_prompt(self, ids):
        a = np.ascontiguousarray(ids, np.int32)
        call("sli_model_set_prompt", self._h, a.ctypes.data_as(ctypes.c_void_p), a.size)

    def state(self, seq: int = 0):
        p, t, a, e = (ctypes.c_int32() for _ in range(4))
        call("sli_model_get_state_seq", self._h, seq, ctypes.byref(p), ctypes.byref(t), ctypes.byref(a),
             ctypes.byref(e))
        return {"pos": p.value, "token": t.value, "last_argmax": a.value, "error": e.value}

    def set_state_seq(self, seq: int, token: int, pos: int, advance: bool = True):
        call("sli_model_set_state_seq", self._h, seq, token, pos, 1 if advance else 0)

    def set_prompt_seq(self, seq: int, ids):
        a = np.ascontiguousarray(ids, np.int32)
        call("sli_model_set_prompt_seq", self._h, seq, a.ctypes.data_as(ctypes.c_void_p), a.size)

    def history(self, seq: int, n: int) -> np.ndarray:
        out = np.empty(n, np.int32)
        call("sli_model_get_history", self._h, seq, n, out.ctypes.data_as(ctypes.c_void_p))
        return out

    @property
    def local_vocab(self) -> int:
        c = self.config
        chunk = -(-c.vocab_size // self.tp_size)
        return max(0, min(chunk, c.vocab_size - self.tp_rank * chunk))

    # ------------------------------------------------------------------ execution
    EXEC = {"launches": 0, "persist": 2}

    def set_exec(self, mode: str) -> "LlamaModel":
        """"launches": one graph of fused launches per layer; "persist": the embedding, every layer as ONE persistent
        launch (csrc/tp_layers.h; batch-1 fp16 models at head_dim 128 whose per-CU shares fit, e.g. the TP-4 / TP-8
        shards of Llama-2-7B; under tensor parallelism after set_allreduce("fused_wg") or without a communicator),
        then the LM head. Any other name (e.g. the removed "persistent") goes to the C layer as an unknown mode, which
        raises SliError(SLI_ERR_ARG) with its message."""
        call("sli_model_set_exec", self._h, self.EXEC.get(mode, -1))
        return self

    def exec_mode(self) -> str:
        v = ctypes.c_int32()
        call("sli_model_get_exec", self._h, ctypes.byref(v))
        return {i: k for k, i in self.EXEC.items()}[v.value]

    # ------------------------------------------------------------------ sampling (sli_model_set_sampling)
    def set_sampling(self, temperature: float | None = None, top_k: int = 0, top_p: float = 1.0,
                     seed: int = 0) -> "LlamaModel":
        """Seeded temperature / top-k / top-p sampling inside the step (the rule: sli.h at sli_sample);
        ``set_sampling(None)`` or temperature 0 goes back to greedy, the default. ``predict*`` follow the state: past
        the prompt they feed what was drawn. Changing the parameters while sampling is on re-captures nothing."""
        if temperature is None:
            call("sli_model_set_sampling", self._h, None)
        else:
            prm = _lib.Sampling(temperature, top_k, top_p, seed & 0xFFFFFFFF)
            call("sli_model_set_sampling", self._h, ctypes.byref(prm))
        return self

    def sampling(self) -> dict | None:
        """The parameters in force, or None while decoding greedily."""
        prm = _lib.Sampling()
        call("sli_model_get_sampling", self._h, ctypes.byref(prm))
        if prm.temperature == 0.0:
            return None
        return {"temperature": prm.temperature, "top_k": prm.top_k, "top_p": prm.top_p, "seed": prm.seed}

    def sampled(self, seq: int = 0) -> int:
        """The token sequence ``seq`` drew in the last step; -1 while sampling is off."""
        v = ctypes.c_int32()
        call("sli_model_get_sampled", self._h, seq, ctypes.byref(v))
        return v.value

    def graph_captures(self) -> int:
        """How many times the step graph has been captured (sli_model_graph_captures)."""
        v = ctypes.c_int32()
        call("sli_model_graph_captures", self._h, ctypes.byref(v))
        return v.value

    # ------------------------------------------------------------------ per-sequence generation (sli_model_set_gen_seq)
    def set_generation(self, seq: int, temperature: float | None = 0.0, top_k: int = 0, top_p: float = 1.0,
                       seed: int = 0, min_p: float = 0.0, repetition_penalty: float = 1.0,
                       presence_penalty: float = 0.0, frequency_penalty: float = 0.0, penalty_from: int = 0,
                       max_pos: int = 0, stop=()) -> "LlamaModel":
        """Sequence ``seq``'s own generation block (the rule: sli.h at sli_sample_gen and sli_model_set_gen_seq):
        sampling, min-p, the three penalties over its history from ``penalty_from`` on, and its stop conditions (up to
        8 ``stop`` tokens; ``max_pos``: the last position it may reach, 0 for none). ``set_generation(seq, None)``
        returns it to the default (greedy, no penalties, no stop). The first call puts the model into per-sequence
        mode; later changes re-capture nothing; any ``set_sampling`` call leaves the mode."""
        if temperature is None:
            call("sli_model_set_gen_seq", self._h, seq, None)
        else:
            from .ops import gen_params
            prm = gen_params(temperature, top_k, top_p, seed, min_p, repetition_penalty, presence_penalty,
                             frequency_penalty, penalty_from, max_pos, stop)
            call("sli_model_set_gen_seq", self._h, seq, ctypes.byref(prm))
        return self

    def generation(self, seq: int) -> dict:
        """Sequence ``seq``'s block in force, as set_generation's keywords."""
        prm = _lib.GenParams()
        call("sli_model_get_gen_seq", self._h, seq, ctypes.byref(prm))
        d = {n: getattr(prm, n) for n, _ in _lib.GenParams._fields_[:10]}
        d["stop"] = tuple(prm.stop[:prm.n_stop])
        return d

    def finished(self) -> np.ndarray:
        """Per sequence: 0 (running or waiting), 1 (it drew one of its stop tokens) or 2 (it reached max_pos or the last
        position): sli_model_get_finished."""
        out = np.zeros(self.batch, np.int32)
        call("sli_model_get_finished", self._h, out.ctypes.data_as(_lib.P_i32))
        return out

    _GEN_KEYS = {"temperature", "top_k", "top_p", "seed", "min_p", "repetition_penalty", "presence_penalty",
                 "frequency_penalty", "penalty_from", "stop"}

    def generate(self, requests) -> list[dict]:
        """Run a queue of requests through the batch. A request is a dict with ``prompt`` (token ids),
        ``max_new_tokens`` and any set_generation keyword (``seed`` defaults to the request's index). Free slots are
        filled from the queue in order (the newly admitted prompts in one prefill_batch call, a one-token prompt
        through set_state_seq), every step is followed by one finished() read, and a finished slot's tokens from
        len(prompt) on are its result, the stop token included. Returns, in request order, ``{"tokens": int32 array,
        "finish": "stop" | "length"}``. The model is left in per-sequence mode with every block cleared. Every request
        is validated (lengths, keywords, the number of stop tokens) before anything runs. A draw is seeded by (seed,
        slot, position), so a sampled request's tokens depend on the slot of the batch it lands in, hence on the
        queue before it; the same call repeats bit for bit, and greedy requests do not depend on their slot."""
        if not self.prefill_batch_ok():
            raise RuntimeError("generate needs a model that takes prefill_batch (prefill_batch_ok())")
        reqs = []
        for i, r in enumerate(requests):
            r = dict(r)
            prompt = [int(t) for t in r.pop("prompt")]
            new = int(r.pop("max_new_tokens"))
            if not prompt or new < 1 or len(prompt) + new > self.config.max_length:
                raise ValueError(f"request {i}: needs a prompt, max_new_tokens >= 1 and len(prompt) + max_new_tokens "
                                 "<= max_len")
            r.setdefault("seed", i)
            unknown = set(r) - self._GEN_KEYS
            if unknown:
                raise ValueError(f"request {i}: unknown keys {sorted(unknown)} (max_pos follows from max_new_tokens)")
            if len(tuple(r.get("stop", ()))) > _lib.MAX_STOP:
                raise ValueError(f"request {i}: at most {_lib.MAX_STOP} stop tokens")
            reqs.append((prompt, new, r))
        results: list = [None] * len(reqs)
        slots: list = [None] * self.batch  # the request each sequence runs
        queue = list(range(len(reqs)))
        for b in range(self.batch):  # nothing runs but what is admitted
            self.set_generation(b, None)
            st = self.state(b)
            self.set_state_seq(b, st["token"], st["pos"], advance=False)
        while queue or any(s is not None for s in slots):
            new_slots = []
            for b in range(self.batch):
                if slots[b] is None and queue:
                    slots[b] = queue.pop(0)
                    new_slots.append(b)
            packed = [b for b in new_slots if len(reqs[slots[b]][0]) > 1]
            if packed:
                self.prefill_batch([reqs[slots[b]][0] for b in packed], packed)
            for b in new_slots:
                prompt, new, kw = reqs[slots[b]]
                if len(prompt) == 1:
                    self.set_prompt_seq(b, prompt)
                    self.set_state_seq(b, prompt[0], 0, advance=True)
                self.set_generation(b, max_pos=len(prompt) - 1 + new, **kw)
            self.step()
            fin = self.finished()
            for b in range(self.batch):
                if slots[b] is None or not fin[b]:
                    continue
                prompt = reqs[slots[b]][0]
                pos = self.state(b)["pos"]
                results[slots[b]] = {"tokens": self.history(b, pos + 1)[len(prompt):].copy(),
                                     "finish": "stop" if fin[b] == _lib.FIN_STOP else "length"}
                slots[b] = None
                self.set_generation(b, None)
        return results

    # ------------------------------------------------------------------ tensor-parallel all-reduce
    def comm_handle(self) -> bytes:
        """This rank's one-shot all-reduce buffer as an IPC handle (exchange it with the other ranks)."""
        n = _lib.load().sli_model_comm_handle_bytes()
        buf = ctypes.create_string_buffer(n)
        call("sli_model_comm_handle", self._h, buf, n)
        return buf.raw

    def comm_open(self, handles: list[bytes]) -> "LlamaModel":
        blob = b"".join(handles)
        buf = ctypes.create_string_buffer(blob, len(blob))
        call("sli_model_comm_open", self._h, buf, len(handles))
        return self

    def set_allreduce(self, mode: str) -> "LlamaModel":
        """"rccl" (ncclAllReduce in the step graph), "oneshot" (oneshot.h, after comm_open), "fused" (the
        one-shot exchange inside the wo / down GEMV launches, batch 1; oneshot.h EpiPush) or "fused_wg" (the
        same per workgroup: ranks on distinct devices, sli.h SLI_ALLREDUCE_FUSED_WG)."""
        call("sli_model_set_allreduce", self._h, {"rccl": 0, "oneshot": 1, "fused": 2, "fused_wg": 3}[mode])
        return self

    # ------------------------------------------------------------------ model.cpp:40-140
    def step(self):
        call("sli_model_step", self._h)

    def sync(self):
        call("sli_model_sync", self._h)

    def logits(self) -> tuple[np.ndarray, int]:
        """This rank's vocab shard of the last step's logits: [local vocab], or [batch, local vocab]."""
        out = np.empty(self.batch * self.local_vocab, np.float32)
        lo = ctypes.c_int32()
        call("sli_model_get_logits", self._h, out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(lo))
        return (out.reshape(self.batch, -1) if self.batch > 1 else out), lo.value

    def forward(self, token: int, pos: int) -> np.ndarray:
        """One decode step at (token, pos); returns this rank's logits shard."""
        self.set_state(token, pos, advance=False)
        self.step()
        return self.logits()[0]

    def forward_batch(self, tokens, positions) -> np.ndarray:
        """One decode step of every sequence b at (tokens[b], positions[b]); returns [batch, local vocab]."""
        for b in range(self.batch):
            self.set_state_seq(b, int(tokens[b]), int(positions[b]), advance=False)
        self.step()
        return self.logits()[0].reshape(self.batch, -1)

    # ------------------------------------------------------------------ model.cpp:142-187
    def predict(self, prompt_ids, max_length: int, want_logits: bool = False):
        """Token ids in: the tokens fed at positions 0..max_length-1 (and the logits). Text in (the reference's
        ``predict(const std::string prompt, int max_length)``): encode it, run the same loop, print and return
        the text model.cpp:154-186 writes — every fed token and the final argmax, decoded one by one."""
        if isinstance(prompt_ids, str):
            return self._predict_text(prompt_ids, max_length)
        p = np.ascontiguousarray(prompt_ids, np.int32)
        toks = np.empty(max_length, np.int32)
        logits = np.empty((max_length, self.local_vocab), np.float32) if want_logits else None
        call("sli_model_predict", self._h, p.ctypes.data_as(ctypes.c_void_p), p.size, max_length,
             toks.ctypes.data_as(ctypes.c_void_p), logits.ctypes.data_as(ctypes.c_void_p) if want_logits else None)
        return (toks, logits) if want_logits else toks

    def _predict_text(self, prompt: str, max_length: int) -> str:
        from .encode import render_predict
        if self.encode_layer is None:
            raise RuntimeError("predict(text) needs a tokenizer_path")
        ids = self.encode_layer.encode(prompt)
        if not ids:
            raise ValueError("the prompt encodes to no tokens")
        if max_length <= 0:  # the loop body never runs: only the first prompt token is printed (model.cpp:154-155)
            text = render_predict(self.encode_layer, [], ids[0])
        else:
            fed = self.predict(ids, max_length)
            text = render_predict(self.encode_layer, fed.reshape(-1, max_length)[0], self.state()["token"])
        print(text, end="")
        return text

    def prefill(self, prompt_ids):
        """Run prompt positions 0..n-2 through the layers in chunks of up to 256 (MFMA GEMM projections,
        block-causal attention) and leave the state at the last prompt token, so the next step() yields the
        first greedy token (sli_model_prefill). Under multi-process tensor parallelism every rank calls it."""
        p = np.ascontiguousarray(prompt_ids, np.int32)
        call("sli_model_prefill", self._h, p.ctypes.data_as(ctypes.c_void_p), p.size)

    def prefill_path(self) -> str:
        """'mfma' (chunked MFMA GEMMs) or 'decode' (teacher-forced decode steps): sli_model_prefill_path."""
        return "mfma" if _lib.load().sli_model_prefill_path(self._h) == 1 else "decode"

    def set_prefill(self, mode: str):
        """Which path the next prefill takes (sli_model_set_prefill): 'auto' (the GEMM prefill where the model can
        take it, MXFP4 weights excepted), 'gemm' (the chunked MFMA prefill; an error where the model cannot take it),
        'decode' (teacher-forced decode steps) or 'gemm-kv8' ('gemm', and also accepted by a model with an FP8 K/V
        cache, which 'gemm' refuses and 'auto' keeps on the decode step). prefill_path() reports the outcome."""
        call("sli_model_set_prefill", self._h, _PREFILL_MODES[mode])

    def fused_qkv_attn(self) -> int:
        """1 when the decode step runs q/k/v + attention as one launch per layer, 0 otherwise:
        sli_model_fused_qkv_attn."""
        return int(_lib.load().sli_model_fused_qkv_attn(self._h))

    def predict_prefill(self, prompt_ids, max_length: int, want_logits: bool = False):
        """predict() with the prompt prefilled; logits rows of positions < len(prompt) - 1 are NaN."""
        p = np.ascontiguousarray(prompt_ids, np.int32)
        toks = np.empty(max_length, np.int32)
        logits = np.empty((max_length, self.local_vocab), np.float32) if want_logits else None
        call("sli_model_predict_prefill", self._h, p.ctypes.data_as(ctypes.c_void_p), p.size, max_length,
             toks.ctypes.data_as(ctypes.c_void_p), logits.ctypes.data_as(ctypes.c_void_p) if want_logits else None)
        return (toks, logits) if want_logits else toks

    def predict_batch(self, prompts, max_length: int, want_logits: bool = False):
        """predict for `batch` sequences with their own prompts (ragged lengths allowed): tokens [batch,
        max_length] (the token fed at each position), logits [batch, max_length, local vocab]."""
        if len(prompts) != self.batch:
            raise ValueError(f"need {self.batch} prompts")
        ld = max(len(p) for p in prompts)
        P = np.zeros((self.batch, ld), np.int32)
        for b, p in enumerate(prompts):
            P[b, :len(p)] = p
        lens = np.array([len(p) for p in prompts], np.int32)
        toks = np.empty((self.batch, max_length), np.int32)
        logits = np.empty((max_length, self.batch, self.local_vocab), np.float32) if want_logits else None
        call("sli_model_predict_batch", self._h, P.ctypes.data_as(ctypes.c_void_p), lens.ctypes.data_as(ctypes.c_void_p),
             ld, max_length, toks.ctypes.data_as(ctypes.c_void_p),
             logits.ctypes.data_as(ctypes.c_void_p) if want_logits else None)
        return (toks, logits.transpose(1, 0, 2).copy()) if want_logits else toks

    @staticmethod
    def _ragged(prompts):
        ld = max(1, max(len(p) for p in prompts))
        P = np.zeros((len(prompts), ld), np.int32)
        for b, p in enumerate(prompts):
            P[b, :len(p)] = p
        return P, np.array([len(p) for p in prompts], np.int32), ld

    def prefill_batch_ok(self) -> bool:
        """Whether this model takes prefill_batch (sli_model_prefill_seqs_ok)."""
        return _lib.load().sli_model_prefill_seqs_ok(self._h) == 1

    def prefill_batch(self, prompts, seqs=None):
        """Prefill sequences ``seqs`` (default 0 .. len(prompts)-1; distinct, < batch) with their own prompts as packed
        MFMA GEMM chunks (sli_model_prefill_seqs); the other sequences keep their cache rows and state. Each listed
        sequence is left at its last prompt token, so the next step() yields its first generated token."""
        seqs = np.arange(len(prompts), dtype=np.int32) if seqs is None else np.ascontiguousarray(seqs, np.int32)
        if seqs.size != len(prompts) or not len(prompts):
            raise ValueError("one prompt per listed sequence")
        P, lens, ld = self._ragged(prompts)
        call("sli_model_prefill_seqs", self._h, seqs.ctypes.data_as(ctypes.c_void_p), seqs.size,
             P.ctypes.data_as(ctypes.c_void_p), lens.ctypes.data_as(ctypes.c_void_p), ld)

    def score_ok(self) -> bool:
        """Whether this model takes score() (sli_model_score_seqs_ok)."""
        return _lib.load().sli_model_score_seqs_ok(self._h) == 1

    def score(self, prompts, seqs=None):
        """prefill_batch(prompts, seqs), and the log-probability of every prompt token given the tokens before it
        (sli_model_score_seqs). One record per prompt: ``logprobs`` (float32), ``top`` (int32: the model's first-max
        token at that place) and ``top_logprobs`` (float32), arrays of length len(prompt) - 1 whose entry t - 1 is
        about prompt[t]. The cache rows, state and history are left as prefill_batch leaves them."""
        seqs = np.arange(len(prompts), dtype=np.int32) if seqs is None else np.ascontiguousarray(seqs, np.int32)
        if seqs.size != len(prompts) or not len(prompts):
            raise ValueError("one prompt per listed sequence")
        P, lens, ld = self._ragged(prompts)
        lp = np.empty((len(prompts), ld), np.float32)
        top = np.empty((len(prompts), ld), np.int32)
        tlp = np.empty((len(prompts), ld), np.float32)
        call("sli_model_score_seqs", self._h, seqs.ctypes.data_as(ctypes.c_void_p), seqs.size,
             P.ctypes.data_as(ctypes.c_void_p), lens.ctypes.data_as(ctypes.c_void_p), ld,
             lp.ctypes.data_as(ctypes.c_void_p), top.ctypes.data_as(ctypes.c_void_p),
             tlp.ctypes.data_as(ctypes.c_void_p))
        return [{"logprobs": lp[i, 1:n].copy(), "top": top[i, 1:n].copy(), "top_logprobs": tlp[i, 1:n].copy()}
                for i, n in enumerate(int(x) for x in lens)]

    def perplexity(self, prompts) -> float:
        """exp(-sum of the prompts' token log-probabilities / number of scored tokens), accumulated in float64."""
        recs = self.score(prompts)
        total = sum(float(np.sum(r["logprobs"], dtype=np.float64)) for r in recs)
        count = sum(len(r["logprobs"]) for r in recs)
        if not count:
            raise ValueError("no scored token: every prompt has length 1")
        return float(np.exp(-total / count))

    # ------------------------------------------------------------------ continuing sequences from a start position
    def _extend_args(self, tokens, seqs, starts):
        if seqs is None and self.batch == 1 and len(tokens) and np.ndim(tokens[0]) == 0:
            tokens = [tokens]  # one flat list for the one sequence of a batch-1 model
        seqs = np.arange(len(tokens), dtype=np.int32) if seqs is None else np.ascontiguousarray(seqs, np.int32)
        if seqs.size != len(tokens) or not len(tokens):
            raise ValueError("one token list per listed sequence")
        if starts is not None:
            starts = np.ascontiguousarray(starts, np.int32)
            if starts.shape != seqs.shape:
                raise ValueError("one start per listed sequence")
        P, counts, ld = self._ragged(tokens)
        return tokens, seqs, starts, P, counts, ld

    def extend(self, tokens, seqs=None, starts=None, advance: bool = True):
        """Continue sequences ``seqs`` (default 0 .. len(tokens)-1) from positions ``starts`` (default: each sequence's
        current position): tokens[i][j] is the token at position starts[i] + j. Rows below a sequence's position are
        taken from its cache, the new rows run as packed MFMA GEMM chunks, and the sequence is left at its last token
        (sli_model_extend_seqs; the models prefill_batch takes). ``advance=False`` leaves the sequences waiting while
        the rest of the batch steps. A batch-1 model outside the packed route (fp32 weights or cache, a TP rank)
        continues through extend_one, which follows set_prefill."""
        tokens, seqs, starts, P, counts, ld = self._extend_args(tokens, seqs, starts)
        call("sli_model_extend_seqs", self._h, seqs.ctypes.data_as(ctypes.c_void_p), seqs.size,
             P.ctypes.data_as(ctypes.c_void_p), starts.ctypes.data_as(ctypes.c_void_p) if starts is not None else None,
             counts.ctypes.data_as(ctypes.c_void_p), ld, 1 if advance else 0)

    def extend_one(self, tokens, start: int | None = None):
        """sli_model_extend: the one-sequence route of a batch-1 model, following set_prefill (the GEMM chunks, or the
        tokens teacher-forced through the decode step from ``start``; default: the current position)."""
        p = np.ascontiguousarray(tokens, np.int32)
        call("sli_model_extend", self._h, p.ctypes.data_as(ctypes.c_void_p), -1 if start is None else int(start), p.size)

    def append(self, tokens, seqs=None):
        """The chat-turn call: append ``tokens[i]`` behind sequence ``seqs[i]``'s pending token. Each sequence's pending
        token and position are read, and the sequence is extended from there with (pending token, *tokens[i]); it is
        left advancing at the last appended token."""
        tokens, seqs, _, _, _, _ = self._extend_args(tokens, seqs, None)
        turn = []
        for s, t in zip(seqs.tolist(), tokens):
            turn.append([self.state(s)["token"], *[int(v) for v in t]])
        self.extend(turn, seqs)

    def score_extend(self, tokens, seqs=None, starts=None):
        """extend(tokens, seqs, starts), and the log-probability of every token but each list's first given everything
        before it (sli_model_score_extend_seqs). Records shaped like score()'s: arrays of length len(tokens[i]) - 1
        whose entry j - 1 is about tokens[i][j]."""
        tokens, seqs, starts, P, counts, ld = self._extend_args(tokens, seqs, starts)
        lp = np.empty((len(tokens), ld), np.float32)
        top = np.empty((len(tokens), ld), np.int32)
        tlp = np.empty((len(tokens), ld), np.float32)
        call("sli_model_score_extend_seqs", self._h, seqs.ctypes.data_as(ctypes.c_void_p), seqs.size,
             P.ctypes.data_as(ctypes.c_void_p), starts.ctypes.data_as(ctypes.c_void_p) if starts is not None else None,
             counts.ctypes.data_as(ctypes.c_void_p), ld, 1, lp.ctypes.data_as(ctypes.c_void_p),
             top.ctypes.data_as(ctypes.c_void_p), tlp.ctypes.data_as(ctypes.c_void_p))
        return [{"logprobs": lp[i, 1:n].copy(), "top": top[i, 1:n].copy(), "top_logprobs": tlp[i, 1:n].copy()}
                for i, n in enumerate(int(x) for x in counts)]

    def fork(self, src: int, dst: int, n: int | None = None):
        """Copy the first ``n`` cache rows (default: all of src's, its position) and history [0, n] of sequence ``src``
        to sequence ``dst`` (sli_model_copy_prefix): dst waits at (src's token at position n, position n) and can be
        extended or appended to from there; src is untouched."""
        call("sli_model_copy_prefix", self._h, src, dst, self.state(src)["pos"] if n is None else n)

    def admit(self, prompts, seqs, max_tokens: int, between=None):
        """Admit ``prompts`` into sequences ``seqs`` of a running batch in calls of at most ``max_tokens`` tokens per
        sequence: extend() from position 0 on, the sequences waiting (advance=False) after every call but the last,
        ``between()`` called after every call but the last (the running sequences' decode steps go there). A call that
        is not a prompt's last ends one token past a multiple of 16 positions, so every call's rows are whole groups."""
        if max_tokens < 2:
            raise ValueError("max_tokens must be at least 2 (a call re-feeds the token the call before left pending)")
        seqs = [int(s) for s in seqs]
        prompts = [[int(v) for v in p] for p in prompts]
        if len(prompts) != len(seqs) or not seqs or any(not p for p in prompts):
            raise ValueError("one non-empty prompt per listed sequence")
        # a call over tokens [lo, hi) fills rows lo .. hi - 2 and leaves token hi - 1 pending: the next call starts there.
        # Where the prompt goes on, hi - 1 is brought down to a multiple of 16, so that the next call's first group is a
        # whole one and a call's groups are not one more than its rows need (a 17th group is a second chunk).
        def end(p, a):
            hi = min(len(p), a + max_tokens)
            cut = (hi - 1) // 16 * 16 + 1
            return cut if hi < len(p) and cut - a >= 2 else hi

        lo, first = [0] * len(seqs), True
        while True:
            hi = [end(p, a) for p, a in zip(prompts, lo)]
            last = all(h == len(p) for h, p in zip(hi, prompts))
            # a sequence whose prompt ended in an earlier call waits (one token from its position changes nothing) and
            # is listed again in the last call, which releases every sequence together
            live = [i for i in range(len(seqs)) if first or last or hi[i] - lo[i] > 1]
            self.extend([prompts[i][lo[i]:hi[i]] for i in live], [seqs[i] for i in live], [lo[i] for i in live],
                        advance=last)
            if last:
                return
            lo, first = [h - 1 for h in hi], False
            if between is not None:
                between()

    def predict_batch_prefill(self, prompts, max_length: int, want_logits: bool = False):
        """predict_batch with the prompts prefilled (sli_model_predict_batch_prefill): tokens [batch, max_length],
        logits [batch, max_length, local vocab] with NaN rows at positions < len(prompt) - 1."""
        if len(prompts) != self.batch:
            raise ValueError(f"need {self.batch} prompts")
        P, lens, ld = self._ragged(prompts)
        toks = np.empty((self.batch, max_length), np.int32)
        logits = np.empty((max_length, self.batch, self.local_vocab), np.float32) if want_logits else None
        call("sli_model_predict_batch_prefill", self._h, P.ctypes.data_as(ctypes.c_void_p),
             lens.ctypes.data_as(ctypes.c_void_p), ld, max_length, toks.ctypes.data_as(ctypes.c_void_p),
             logits.ctypes.data_as(ctypes.c_void_p) if want_logits else None)
        return (toks, logits.transpose(1, 0, 2).copy()) if want_logits else toks

    def weight_shard(self, kind: int, index: int = 0) -> np.ndarray:
        """This rank's shard of a weight (sli_tp_plan window) read back as fp32."""
        from .tp import KINDS, shard_window
        name = {v: k for k, v in KINDS.items()}[kind]
        if name == "norm":
            shape = (self.config.hidden_size,)
        else:
            w = shard_window(self.config, name, self.tp_rank, self.tp_size)
            shape = (w.n_rows, w.n_cols)
        out = np.empty(shape, np.float32)
        call("sli_model_get_weight", self._h, kind, index, out.ctypes.data_as(ctypes.c_void_p), out.size)
        return out

    def kv(self, layer: int, which: int, upto: int, seq: int = 0) -> np.ndarray:
        c = self.config
        out = np.empty((upto, c.num_key_value_heads // self.tp_size * c.head_dim), np.float32)
        call("sli_model_get_kv_seq", self._h, seq, layer, which, upto, out.ctypes.data_as(ctypes.c_void_p))
        return out

    # ------------------------------------------------------------------ measurement
    def stream(self) -> int:
        s = ctypes.c_void_p()
        call("sli_model_stream", self._h, ctypes.byref(s))
        return s.value or 0

    def step_bytes(self) -> tuple[float, float]:
        w, k = ctypes.c_double(), ctypes.c_double()
        call("sli_model_step_bytes", self._h, ctypes.byref(w), ctypes.byref(k))
        return w.value, k.value

    def time_steps(self, iters: int = 20) -> float:
        """Mean device µs of one replayed step (HIP events on the model's stream)."""
        v = ctypes.c_double()
        call("sli_model_time_steps", self._h, iters, ctypes.byref(v))
        return v.value

    FAMILIES = ("qkv", "attention", "wo", "gate_up", "down", "lm_head")

    def time_families(self, iters: int = 20) -> dict:
        """Per kernel family: mean device µs per launch, algorithmic bytes per launch, launches per step."""
        n = len(self.FAMILIES)
        us, b, k = (ctypes.c_double * n)(), (ctypes.c_double * n)(), (ctypes.c_int32 * n)()
        call("sli_model_time_families", self._h, iters, us, b, k)
        return {f: {"avg_us": us[i], "bytes_per_launch": b[i], "launches_per_step": k[i]}
                for i, f in enumerate(self.FAMILIES)}

    def time_stream(self, iters: int = 20) -> dict:
        """Per kernel family: mean device µs of a pure streaming read of the same buffers (the floor)."""
        n = len(self.FAMILIES)
        us = (ctypes.c_double * n)()
        call("sli_model_time_stream", self._h, iters, us)
        return {f: us[i] for i, f in enumerate(self.FAMILIES)}

    def time_gemv(self, iters: int = 20) -> dict:
        us, b, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int32()
        call("sli_model_time_gemv", self._h, iters, ctypes.byref(us), ctypes.byref(b), ctypes.byref(n))
        return {"avg_us": us.value, "bytes_per_launch": b.value, "launches_per_step": n.value}


def comm_id() -> bytes:
    """A fresh RCCL unique id (rank 0 creates it and broadcasts it to the other ranks)."""
    n = _lib.load().sli_comm_id_bytes()
    buf = ctypes.create_string_buffer(n)
    call("sli_comm_get_id", buf)
    return buf.raw


class TPGroup:
    """In-process tensor parallelism (sli_tp_group): ``tp_size`` rank engines on one
    device, stepped in lockstep by one graph whose all-reduces are device-side reductions over the ranks'
    buffers. ``ranks[r]`` is a borrowed ``LlamaModel`` of rank r (weights, state, logits shard)."""

    def __init__(self, config: LlamaModelConfig, tp_size: int, w_dtype: str = "f16", kv_dtype: str = "f16",
                 act_mode: int = 0, device: int = 0, seed: int | None = None, batch: int = 1,
                 model_path: str = "", mx_batch: bool = False):
        self.config, self.tp_size, self.batch = config, tp_size, batch
        proto = LlamaModel(model_path=model_path, config=config, w_dtype=w_dtype, kv_dtype=kv_dtype,
                           act_mode=act_mode, tp_rank=0, tp_size=tp_size, device=device, seed=seed, batch=batch)
        mc = proto._config_struct()
        g = ctypes.c_void_p()
        if mx_batch:
            call("sli_tp_group_create_flags", ctypes.byref(mc), tp_size, CREATE_MX_BATCH, ctypes.byref(g))
        else:
            call("sli_tp_group_create", ctypes.byref(mc), tp_size, ctypes.byref(g))
        self._g = g
        self.ranks = []
        for r in range(tp_size):
            h = ctypes.c_void_p()
            call("sli_tp_group_rank", g, r, ctypes.byref(h))
            m = LlamaModel(model_path=model_path, config=config, w_dtype=w_dtype, kv_dtype=kv_dtype,
                           act_mode=act_mode, tp_rank=r, tp_size=tp_size, device=device, seed=seed, batch=batch,
                           mx_batch=mx_batch)
            m._h = h
            m._borrowed = True
            self.ranks.append(m)

    def init(self) -> "TPGroup":
        for m in self.ranks:
            m._load_weights()
        return self

    def close(self):
        if self._g is not None:
            for m in self.ranks:
                m._h = None
            _lib.load().sli_tp_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def fill_kv_synthetic(self, seed: int, upto: int):
        for m in self.ranks:
            m.fill_kv_synthetic(seed, upto)

    def step(self):
        call("sli_tp_group_step", self._g)

    def sync(self):
        call("sli_tp_group_sync", self._g)

    def logits(self) -> np.ndarray:
        """The full-vocabulary logits of the last step ([vocab] or [batch, vocab]), the ranks' shards in place."""
        parts = [m.logits()[0] for m in self.ranks]
        return np.concatenate(parts, axis=-1)

    def forward_batch(self, tokens, positions) -> np.ndarray:
        for m in self.ranks:
            for b in range(self.batch):
                m.set_state_seq(b, int(tokens[b]), int(positions[b]), advance=False)
        self.step()
        return self.logits().reshape(self.batch, -1)

    def forward(self, token: int, pos: int) -> np.ndarray:
        return self.forward_batch([token] * self.batch, [pos] * self.batch)[0]

    def predict_batch(self, prompts, max_length: int, want_logits: bool = False):
        if len(prompts) != self.batch:
            raise ValueError(f"need {self.batch} prompts")
        ld = max(len(p) for p in prompts)
        P = np.zeros((self.batch, ld), np.int32)
        for b, p in enumerate(prompts):
            P[b, :len(p)] = p
        lens = np.array([len(p) for p in prompts], np.int32)
        toks = np.empty((self.batch, max_length), np.int32)
        V = self.config.vocab_size
        logits = np.empty((max_length, self.batch, V), np.float32) if want_logits else None
        call("sli_tp_group_predict_batch", self._g, P.ctypes.data_as(ctypes.c_void_p),
             lens.ctypes.data_as(ctypes.c_void_p), ld, max_length, toks.ctypes.data_as(ctypes.c_void_p),
             logits.ctypes.data_as(ctypes.c_void_p) if want_logits else None)
        return (toks, logits.transpose(1, 0, 2).copy()) if want_logits else toks

    def set_prefill(self, mode: str):
        """LlamaModel.set_prefill for every rank (sli_tp_group_set_prefill)."""
        call("sli_tp_group_set_prefill", self._g, _PREFILL_MODES[mode])

    def prefill_path(self) -> str:
        return self.ranks[0].prefill_path()

    def prefill(self, prompt_ids):
        """sli_tp_group_prefill: the ranks' prefill chunks in lockstep (batch-1 groups)."""
        p = np.ascontiguousarray(prompt_ids, np.int32)
        call("sli_tp_group_prefill", self._g, p.ctypes.data_as(ctypes.c_void_p), p.size)

    def extend(self, tokens, start: int | None = None):
        """sli_tp_group_extend: continue the group's sequence from ``start`` (default: its current position) with
        ``tokens``, tokens[j] at position start + j, on the route prefill() takes (batch-1 groups)."""
        p = np.ascontiguousarray(tokens, np.int32)
        call("sli_tp_group_extend", self._g, p.ctypes.data_as(ctypes.c_void_p), -1 if start is None else int(start),
             p.size)

    def fork(self, src: int, dst: int, n: int | None = None):
        """LlamaModel.fork on every rank's shard of the cache (sli_tp_group_copy_prefix)."""
        call("sli_tp_group_copy_prefix", self._g, src, dst, self.ranks[0].state(src)["pos"] if n is None else n)

    def predict_prefill(self, prompt_ids, max_length: int, want_logits: bool = False):
        """predict() with the prompt prefilled; logits [max_length, vocab], rows < len(prompt) - 1 NaN."""
        p = np.ascontiguousarray(prompt_ids, np.int32)
        toks = np.empty(max_length, np.int32)
        logits = np.empty((max_length, self.config.vocab_size), np.float32) if want_logits else None
        call("sli_tp_group_predict_prefill", self._g, p.ctypes.data_as(ctypes.c_void_p), p.size, max_length,
             toks.ctypes.data_as(ctypes.c_void_p), logits.ctypes.data_as(ctypes.c_void_p) if want_logits else None)
        return (toks, logits) if want_logits else toks

    def predict(self, prompt_ids, max_length: int, want_logits: bool = False):
        r = self.predict_batch([list(prompt_ids)] * self.batch, max_length, want_logits)
        if want_logits:
            return r[0][0], r[1][0]
        return r[0]
