#!/usr/bin/env python3
"""splainference — the completion sidecar, on the MI355X causal decoder.

Contract kept from the reference daemon (/root/reference/splainference.cpp):
  argv    [--oneshot] [--n-ctx N] [--system-prompt-key KEY] <bus> <gguf> <group>  (:410-454)
  labels  0x1000000000000000 WAITING (client posts + bumps) ->
          0x2000000000000000 SERVICING (set before the first token, :232-234) ->
          0x4000000000000000 READY (on completion or failure, :390-392)
  request odd epoch = skip (writer active); the value is read with an epoch
          check (:191-210); the slot is overwritten with the formatted prompt
          (:269) and the completion is APPENDED as it streams: a flush at a
          word boundary (piece starts with ' ' or contains '\\n') or every 8
          tokens (:86, :102-109, :332-364), truncated at max_val_sz (:336-345)
  prompt  the GGUF chat template's family is detected by its markers (chatml, llama 3,
          gemma, phi 3, zephyr, llama 2 / mistral), as llama_chat_apply_template does;
          otherwise the reference's bare fallback "<system>/<user>/<assistant>" (:132-169)
  shard   0x5F1A WILLNEED prio 200, re-bid every 32 appended tokens, WILLNEED
          madvise of the request slot (:39-62, :222-230, :359-363)
  done    ctime backfill with the processing delta (:282, :383-387), "__debug"
          chatter (:94-100), cold-start sweep of WAITING keys (:542-551), then
          poll the signal group every 50 ms (:570-592)
Extra flags: --random-init (no GGUF: random llama weights, byte vocabulary,
printable-byte sampling), --max-tokens (cap per request), --seed, --batch N
(GPU: up to N requests decoded together, one shared step per token; default 1), --prefill-chunk C (with
--batch: WAITING requests are admitted together, C prompt tokens of each per pass; default 0, one whole
prompt at a time), --prefix-cache (with --batch and --prefill-chunk C: the cache rows of the prompt head every
request shares, the system prompt, are computed once and copied into each later request's cache; reuse is
floor(head tokens / C) * C tokens, so pick C no larger than the system prompt).
"""
from __future__ import annotations

import argparse
import os
import signal
import sys
import time
from typing import List, Optional

LABEL_WAITING = 0x1000000000000000
LABEL_SERVICING = 0x2000000000000000
LABEL_READY = 0x4000000000000000
SHARD_ID = 0x5F1A
SHARD_DUR_LIVE = 1 << 30
SHARD_PRIO_LIVE = 200
SHARD_REBID_TOKENS = 32
TOKEN_FLUSH_MAX = 8
POSIX_MADV_WILLNEED = 3
INTENT_WILLNEED = 1

_running = True


def _stop(*_):
    global _running
    _running = False


def debug_post(store, msg: str) -> None:
    line = msg + "\n"
    try:
        store.append("__debug", line)
    except OSError:
        try:
            store.set("__debug", line)
        except OSError:
            pass


def build_prompt(system_msg: str, user_msg: str, template: Optional[str] = None) -> str:
    """The reference renders the model's GGUF chat template with llama_chat_apply_template and
    falls back to a bare "<system>/<user>/<assistant>" layout (splainference.cpp:132-169).
    llama.cpp recognises templates by marker substrings rather than evaluating the jinja; the
    families below follow the same detection, anything else takes the bare fallback."""
    t = template or ""
    sys_ = system_msg
    if "<|im_start|>" in t:  # chatml
        out = f"<|im_start|>system\n{sys_}<|im_end|>\n" if sys_ else ""
        return out + f"<|im_start|>user\n{user_msg}<|im_end|>\n<|im_start|>assistant\n"
    if "<|start_header_id|>" in t:  # llama 3
        out = f"<|start_header_id|>system<|end_header_id|>\n\n{sys_}<|eot_id|>" if sys_ else ""
        return out + (f"<|start_header_id|>user<|end_header_id|>\n\n{user_msg}<|eot_id|>"
                      "<|start_header_id|>assistant<|end_header_id|>\n\n")
    if "<start_of_turn>" in t:  # gemma: the system text is prepended to the user turn
        body = f"{sys_}\n\n{user_msg}" if sys_ else user_msg
        return f"<start_of_turn>user\n{body}<end_of_turn>\n<start_of_turn>model\n"
    if "<|assistant|>" in t and "<|end|>" in t:  # phi 3
        out = f"<|system|>\n{sys_}<|end|>\n" if sys_ else ""
        return out + f"<|user|>\n{user_msg}<|end|>\n<|assistant|>\n"
    if "<|user|>" in t and "</s>" in t:  # zephyr
        out = f"<|system|>\n{sys_}</s>\n" if sys_ else ""
        return out + f"<|user|>\n{user_msg}</s>\n<|assistant|>\n"
    if "[INST]" in t:  # llama 2 / mistral
        if sys_:
            return f"[INST] <<SYS>>\n{sys_}\n<</SYS>>\n\n{user_msg} [/INST]"
        return f"[INST] {user_msg} [/INST]"
    out = ""
    if system_msg:
        out += "<system>\n" + system_msg + "\n"
    return out + "<user>\n" + user_msg + "\n<assistant>\n"


def shared_prompt_prefix(tok, system_msg: str, template: Optional[str] = None) -> List[int]:
    """The tokens every request's prompt starts with under this system prompt and template: two prompts whose
    user messages differ from their first character, tokenised, and their longest common token prefix.  That
    holds for every template family, gemma's included, where the system text sits inside the user turn.  It is
    a hint only: the engine compares the ids of each request, so a request that tokenises differently at the
    seam just misses."""
    a = tok.encode(build_prompt(system_msg, "What is it?", template))
    b = tok.encode(build_prompt(system_msg, "tell me more", template))
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return list(a[:n])


def is_word_boundary(piece: bytes) -> bool:
    return bool(piece) and (piece[:1] in (b" ", b"\n") or b"\n" in piece)


class CompletionStream:
    """The streaming state of one request: tokens become pieces, pieces gather in a chunk, the chunk is
    appended to the slot at a word boundary or every TOKEN_FLUSH_MAX tokens, truncated when the slot is full,
    with the shard re-bid cadence (reference :332-364).  ``take`` a sampled token, produce the next one, then
    ``flush_if_due``; ``close`` writes what is left."""

    def __init__(self, store, tok, key: str, written: int, budget: int):
        self.store, self.tok, self.key = store, tok, key
        self.written, self.left = written, budget
        self.chunk, self.run, self.rebid, self.oom, self.piece = b"", 0, 0, False, b""

    def take(self, t: int) -> bool:
        """False: the completion is over (token budget, or EOS / EOT / end-of-turn: llama_vocab_is_eog,
        reference :310)."""
        if self.left <= 0 or self.tok.is_eog(t):
            return False
        self.left -= 1
        self.piece = self.tok.piece(t)
        self.chunk += self.piece
        self.run += 1
        return True

    def flush_if_due(self) -> bool:
        """False: the slot is full and the completion was truncated."""
        s, key = self.store, self.key
        if (is_word_boundary(self.piece) or self.run >= TOKEN_FLUSH_MAX) and self.chunk:
            if self.written + len(self.chunk) > s.max_val:
                debug_post(s, f"[splainference][WARN]: Slot full, truncating completion: {key}")
                if s.max_val - self.written > 0:
                    s.append(key, self.chunk[: s.max_val - self.written])
                self.oom = True
                return False
            self.written = s.append(key, self.chunk)
            self.chunk, self.run = b"", 0
            self.rebid += TOKEN_FLUSH_MAX
            if self.rebid >= SHARD_REBID_TOKENS:
                s.shard_rebid(SHARD_ID, INTENT_WILLNEED, SHARD_PRIO_LIVE, SHARD_DUR_LIVE)
                self.rebid = 0
        return True

    def close(self) -> None:
        s = self.store
        if self.chunk and not self.oom and s.max_val - self.written > 0:
            s.append(self.key, self.chunk[: s.max_val - self.written])


class Splainference:
    def __init__(self, store, model, tokenizer, sampler, system_prompt_key=None, max_tokens: int = 256,
                 batch: int = 1, prefill_chunk: int = 0, prefix_cache: bool = False):
        self.store, self.model, self.tok, self.sampler = store, model, tokenizer, sampler
        self.system_prompt_key = system_prompt_key
        self.max_tokens = max_tokens
        self.engine = None
        self.batch_engine = None
        gpu = getattr(model, "hip", False) and getattr(model, "decode_kernel", True)
        if batch > 1 and not gpu:
            print(f"[Warn]: --batch {batch} needs the GPU decode kernels; serving one request at a time.", flush=True)
            batch = 1
        if gpu and batch > 1 and getattr(getattr(model, "cfg", None), "experts", 0):
            print(f"[Warn]: --batch {batch} has no mixture-of-experts decode step; serving one request at a time.",
                  flush=True)
            batch = 1
        if gpu and batch > 1:
            from ..models.decoder import BatchDecodeEngine
            self.batch_engine = BatchDecodeEngine(model, batch, sampler.top_p, sampler.temp, sampler.seed,
                                                  sampler.mask)
        elif gpu:
            from ..models.decoder import DecodeEngine
            self.engine = DecodeEngine(model, sampler.top_p, sampler.temp, sampler.seed, sampler.mask)
        # --prefill-chunk C: batched, chunked admission (BatchDecodeEngine.submit / prefill) where the batch
        # engine serves and the prefill kernels take the head dim; ignored wherever serving is sequential
        self.prefill_chunk = prefill_chunk if self.batch_engine is not None and model.prefill_kernel else 0
        # --prefix-cache: BatchDecodeEngine.set_prefix with the prompt head the system prompt gives every request;
        # it rides on the chunked admission, so it is ignored wherever --prefill-chunk is
        self.prefix_cache = bool(prefix_cache) and self.prefill_chunk > 0
        self._prefix_src: Optional[str] = None  # the system prompt value the engine's prefix was built from

    def _read_request(self, key: str):
        s = self.store
        start = s.epoch(key)
        if start & 1:
            debug_post(s, f"[splainference][SKIP]: {key} has odd epoch (writer active).")
            return None, start
        raw = s.raw(key) if s.backend != "hbm" else None
        if raw is not None:
            view, ep = raw
            val = bytes(view)
            if ep != start or s.epoch(key) != start:
                debug_post(s, f"[splainference][SKIP]: {key} epoch shifted during read.")
                return None, start
        else:
            val = s.get(key) or b""
            if s.epoch(key) != start:
                debug_post(s, f"[splainference][SKIP]: {key} epoch shifted during read.")
                return None, start
        if not val:
            debug_post(s, f"[splainference][SKIP]: {key} is empty.")
            return None, start
        return val.decode("utf-8", "replace"), start

    def _finish(self, key: str) -> None:
        self.store.unset_label(key, LABEL_SERVICING)
        self.store.set_label(key, LABEL_READY)
        self.store.bump(key)

    def _begin(self, key: str):
        """Read the request, flip WAITING -> SERVICING and write the formatted prompt into the slot:
        (start epoch, prompt token ids, bytes written, start time), or None when the key is skipped or failed."""
        s = self.store
        user_msg, start = self._read_request(key)
        if user_msg is None:
            return None
        system_msg = ""
        if self.system_prompt_key:
            v = s.get(self.system_prompt_key)
            system_msg = v.decode("utf-8", "replace") if v else ""
        prompt = build_prompt(system_msg, user_msg, getattr(self.tok, "chat_template", None))
        debug_post(s, f"[splainference][START]: Processing key: {key}")
        s.shard_rebid(SHARD_ID, INTENT_WILLNEED, SHARD_PRIO_LIVE, SHARD_DUR_LIVE)
        try:
            s.madvise(SHARD_ID, POSIX_MADV_WILLNEED, 0)
        except OSError:
            pass
        s.unset_label(key, LABEL_WAITING)
        s.set_label(key, LABEL_SERVICING)
        s.bump(key)
        ids = self.tok.encode(prompt)
        if not ids:
            debug_post(s, f"[splainference][ERROR]: Tokenization failed for key: {key}")
            self._finish(key)
            return None
        pb = prompt.encode("utf-8")[: s.max_val]
        s.set(key, pb)
        t0 = time.perf_counter_ns()
        if self.model.cfg.n_ctx - len(ids) <= 0:
            debug_post(s, f"[splainference][ERROR]: Prefill decode failed for key: {key}")
            self._finish(key)
            return None
        return start, ids, len(pb), t0

    def _done(self, key: str, t0: int) -> None:
        from ..store import TIME_CTIME
        s = self.store
        s.set_time(key, TIME_CTIME, int(time.time()), (time.perf_counter_ns() - t0) // 1000)
        self._finish(key)
        debug_post(s, f"[splainference][DONE]: Completion written to key: {key}")

    def process(self, key: str) -> int:
        began = self._begin(key)
        if began is None:
            return 0
        start, ids, written, t0 = began
        self.model.reset()
        ctx_room = self.model.cfg.n_ctx - len(ids)
        eng = self.engine
        if eng is not None:  # GPU: prefill + device sampler, then one graph replay per token
            t = eng.first_token(ids)
        else:
            logits = self.model.forward(ids)
        out = CompletionStream(self.store, self.tok, key, written, min(self.max_tokens, ctx_room))
        while _running and out.left > 0:
            if eng is None:
                t = self.sampler(logits)
            if not out.take(t):
                break
            if eng is not None:
                t = eng.next_token()
            else:
                logits = self.model.forward([t])
            if not out.flush_if_due():
                break
        out.close()
        self._done(key, t0)
        return start

    def serve_batch(self) -> int:
        """--batch N: decode up to N requests together until no key is WAITING and none is in flight.  Between
        two shared steps WAITING keys are admitted into free slots (their prefill stalls the others for its
        duration; with --prefill-chunk C they are submitted instead and one pass over the next C prompt tokens
        of every submitted request runs before each step, a request's stream starting when its first token
        arrives; with --prefix-cache the engine's shared prefix follows the system prompt key, re-read whenever
        nothing is pending); after a step every request streams its own token.  A request's seed is the daemon
        seed XOR the key's hash, so its completion does not depend on what shares its steps.  Returns requests
        served."""
        eng = self.batch_engine
        live = {}  # slot -> [key, stream, t0, next token]
        pend = {}  # slot -> (key, prompt tokens, bytes written, t0): submitted, first token not drawn yet
        served = 0
        chunk = self.prefill_chunk

        def finish(slot):
            key, out, t0, _ = live.pop(slot)
            out.close()
            eng.release(slot)
            self._done(key, t0)

        while True:
            if self.prefix_cache and self.system_prompt_key and not pend:
                v = self.store.get(self.system_prompt_key)
                system_msg = v.decode("utf-8", "replace") if v else ""
                if system_msg != self._prefix_src:
                    head = shared_prompt_prefix(self.tok, system_msg, getattr(self.tok, "chat_template", None))
                    # a head that fills the context serves no request: nothing to reuse
                    eng.set_prefix(head if len(head) < self.model.cfg.n_ctx else None, chunk)
                    self._prefix_src = system_msg
            if _running:
                for key in self.waiting():
                    if len(live) + len(pend) >= eng.S or not _running:
                        break
                    began = self._begin(key)
                    if began is None:
                        continue
                    _, ids, written, t0 = began
                    from ..store import hash_key
                    seed = self.sampler.seed ^ hash_key(key)
                    served += 1
                    if chunk > 0:  # --prefill-chunk: reserve the slot now, prefill with the others below
                        pend[eng.submit(ids, seed=seed)] = (key, len(ids), written, t0)
                        continue
                    slot, t = eng.admit(ids, seed=seed)
                    budget = min(self.max_tokens, self.model.cfg.n_ctx - len(ids))
                    live[slot] = [key, CompletionStream(self.store, self.tok, key, written, budget), t0, t]
            elif pend:
                # shutdown: a pending request has produced nothing yet.  It is cancelled and closed the way a
                # live one is: SERVICING -> READY with the formatted prompt and an empty completion, so no key
                # is left SERVICING with no daemon behind it
                for slot in list(pend):
                    key, _, _, t0 = pend.pop(slot)
                    eng.release(slot)
                    self._done(key, t0)
            if pend:
                # one pass over the next chunk of every pending prompt, then one step for the live slots
                for slot, t in eng.prefill(chunk).items():
                    key, n, written, t0 = pend.pop(slot)
                    budget = min(self.max_tokens, self.model.cfg.n_ctx - n)
                    live[slot] = [key, CompletionStream(self.store, self.tok, key, written, budget), t0, t]
            if not live:
                if pend:
                    continue
                if self.prefix_cache:
                    print(f"[splainference] prefix cache: {eng.prefix_hits} hits, {eng.prefix_rows_reused} rows "
                          "reused", flush=True)
                return served
            for slot in list(live):
                if not _running or not live[slot][1].take(live[slot][3]):
                    finish(slot)
            if not live:
                continue
            toks = eng.step()
            for slot in list(live):
                live[slot][3] = toks[slot]
                if not live[slot][1].flush_if_due():
                    finish(slot)

    def waiting(self):
        return [k for k, _ in self.store.enumerate(LABEL_WAITING)]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="splainference")
    ap.add_argument("--oneshot", action="store_true")
    ap.add_argument("--n-ctx", type=int, default=0)
    ap.add_argument("--system-prompt-key", default=None)
    ap.add_argument("--random-init", action="store_true")
    ap.add_argument("--max-tokens", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0xFFFFFFFF)
    ap.add_argument("--poll-ms", type=int, default=50)
    ap.add_argument("--batch", type=int, default=1,
                    help="GPU: decode up to N (2..16) requests together, one shared step per token; 1 (default) "
                         "serves one request at a time")
    ap.add_argument("--prefill-chunk", type=int, default=0,
                    help="with --batch on the GPU: admit WAITING requests together, C prompt tokens of each per "
                         "pass, one pass between two decode steps; 0 (default) prefills one whole prompt at a time")
    ap.add_argument("--prefix-cache", action="store_true",
                    help="with --batch >= 2 and --prefill-chunk C > 0: compute the cache rows of the prompt head "
                         "every request shares (the --system-prompt-key text) once and copy them into each later "
                         "request; floor(head / C) * C tokens are reused, so pick C no larger than the system prompt")
    ap.add_argument("--device", default=None, help="cuda (default when a GPU is present) or cpu")
    ap.add_argument("--quant", default="auto", choices=["auto", "bf16", "q4"],
                    help="weights in HBM: q4 = 4-bit Q4G32 (decode streams 0.625 B per weight), bf16, or auto "
                         "(q4 for a 4-bit GGUF, bf16 otherwise; --random-init: bf16)")
    ap.add_argument("bus")
    ap.add_argument("gguf")
    ap.add_argument("group", type=int)
    a = ap.parse_args(argv)
    if not 0 <= a.group < 64:
        print("Error: signal_group_id must be 0-63.", file=sys.stderr)
        return 1
    if not 1 <= a.batch <= 16:
        print("Error: --batch must be 1-16.", file=sys.stderr)
        return 1
    if a.prefill_chunk < 0:
        print("Error: --prefill-chunk must be >= 0.", file=sys.stderr)
        return 1
    if a.prefix_cache and (a.batch < 2 or a.prefill_chunk <= 0):
        print("Error: --prefix-cache needs --batch >= 2 and --prefill-chunk > 0.", file=sys.stderr)
        return 1
    import torch
    from ..store import Store
    from ..models.decoder import ByteTokenizer, CausalLM, DecoderConfig, Sampler
    signal.signal(signal.SIGINT, _stop)
    signal.signal(signal.SIGTERM, _stop)
    try:
        store = Store.open(a.bus)
    except OSError:
        print(f"Failed to connect to Splinter bus: {a.bus}", file=sys.stderr)
        return 1
    try:
        store.shard_claim(SHARD_ID, INTENT_WILLNEED, SHARD_PRIO_LIVE, SHARD_DUR_LIVE)
    except OSError:
        print("[Warn]: could not claim a shard bid slot (table full?); continuing without cooperative advisement.")
    device = a.device or ("cuda" if torch.cuda.is_available() else "cpu")
    print(f"[Startup]: Loading {'random-init decoder' if a.random_init else 'GGUF model `' + a.gguf + '`'} "
          f"on {device} ...", flush=True)
    if a.random_init:
        cfg = DecoderConfig()
        if a.n_ctx > 0:
            cfg.n_ctx = a.n_ctx
        q = "q4" if a.quant == "q4" and device != "cpu" else "bf16"
        model, tok = CausalLM.random(cfg, device=device, quant=q), ByteTokenizer()
    else:
        try:
            model, tok = CausalLM.from_gguf(a.gguf, device=device, quant=a.quant)
        except ValueError as e:  # an architecture or rope layout the decoder does not compute: refuse to serve
            print(f"Error: cannot serve `{a.gguf}`: {e}", file=sys.stderr)
            store.shard_release(SHARD_ID)
            store.close()
            return 1
        if a.n_ctx > 0:
            model.cfg.n_ctx = min(a.n_ctx, model.cos.shape[0])
    print(f"[Startup]: context window = {model.cfg.n_ctx} tokens, {model.quant} weights.", flush=True)
    sampler = Sampler(seed=a.seed, mask=tok.printable_mask(model.cfg.vocab))
    d = Splainference(store, model, tok, sampler, a.system_prompt_key, a.max_tokens, a.batch, a.prefill_chunk,
                      a.prefix_cache)
    pending = d.waiting()
    if pending:
        print(f"[Startup]: {len(pending)} waiting key(s) found at cold start.", flush=True)
        if d.batch_engine is not None:
            d.serve_batch()
        else:
            for k in pending:
                d.process(k)
    if a.oneshot:
        store.shard_release(SHARD_ID)
        store.close()
        return 0
    last = store.signal_count(a.group)
    print(f"[Active]: Watching signal group {a.group} (count: {last})", flush=True)
    debug_post(store, "[splainference][Active]: Completion daemon online.")
    while _running:
        cur = store.signal_count(a.group)
        if cur == last:
            time.sleep(a.poll_ms / 1e3)
            continue
        if d.batch_engine is not None:
            d.serve_batch()
        else:
            for k in d.waiting():
                if not _running:
                    break
                d.process(k)
        last = cur
    print("\n[Signal]: Shutting down splainference safely...")
    debug_post(store, "[splainference]: Daemon shutting down.")
    store.shard_release(SHARD_ID)
    store.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
