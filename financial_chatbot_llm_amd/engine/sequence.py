"""Request / sequence state for the continuous-batching engine."""
from __future__ import annotations

import contextvars
import enum
import itertools
import time
from dataclasses import dataclass, field
from typing import List, Optional, Sequence as Seq, Tuple


# Start of the user turn a request belongs to (time.perf_counter), set by the serving layer for
# everything the turn awaits (serving.worker): the scheduler orders prefill work by it, so a
# turn's respond prefill -- already a decide call deep into its TTFT -- is not queued behind the
# decide prefills of turns that arrived after it.
TURN_START: contextvars.ContextVar = contextvars.ContextVar("penny_turn_start", default=None)


@dataclass
class SamplingParams:
    temperature: float = 0.5            # reference: llm_agent.py:37,44
    top_k: int = 0                      # 0 = disabled
    top_p: float = 1.0
    max_tokens: int = 256
    ignore_eos: bool = False            # benchmarks force fixed decode lengths
    stop_token_ids: Seq[int] = ()
    seed: Optional[int] = None
    forced_output: Optional[List[int]] = None   # teacher-forced continuation (scripted tool calls)
    # jump-forward decoding (agent.grammar): forced_jump[k] -- output token k is forced by the
    # output grammar given tokens[:k], so it is appended with its predecessor instead of being
    # sampled; grammar -- the same oracle for sampled outputs (``forced(text) -> (str, ends)``)
    forced_jump: Optional[List[bool]] = None
    grammar: Optional[object] = None
    # KV retention hint: the prompt's uncached part will not recur (e.g. the respond prompt around
    # a one-off retrieval context), so its blocks are recycled before any other cached block
    ephemeral_kv: bool = False
    # prompt-lookup speculative decoding (engine.speculative): up to this many draft tokens copied
    # from the prompt are verified per step (0 = off)
    prompt_lookup: int = 0
    priority_ts: Optional[float] = None   # scheduling time (TURN_START); None: the request's arrival
    # constrained decoding (agent.automaton.TokenAutomaton): every SAMPLED token keeps the output
    # inside the automaton's language (the device sampler masks the rest); teacher-forced outputs
    # (forced_output) sample nothing and ignore it.  TP = 1 without CP only.
    constraint: Optional[object] = None
    # report each sampled token's log-probability (Sequence.output_logprobs, StepOutput.new_logprobs):
    # log softmax of the raw bf16 logits at temperature 1 -- the quantity score() reports; the
    # temperature, top-k / top-p and the constraint choose the token, not the number.  Never changes a
    # token.  TP = 1 without CP only.
    logprobs: bool = False
    # also report, per sampled token, the N most likely tokens of the same raw distribution with their
    # log-probabilities (Sequence.output_top_logprobs, StepOutput.new_top_logprobs): 0 (off) .. 20,
    # implies ``logprobs``.  Descending, equal logits by ascending token id; no mask, penalty or
    # top-k / top-p applies.  Never changes a token; steps holding such a row pay one LM-head logits
    # GEMM where they would sample inside the fused LM head.  TP = 1 without CP only.
    top_logprobs: int = 0
    # penalties on tokens the sequence holds already (ops.penalty), applied to the logits in front of
    # the automaton mask, top-k / top-p and the sampler: repetition divides a positive (multiplies a
    # negative) logit of every token in the prompt or the output; presence is subtracted once and
    # frequency once per occurrence, for tokens of the output only.  Neutral: 1, 0, 0.  A scripted
    # output (forced_output) ignores them; a penalised request proposes no prompt-lookup drafts and
    # needs max_tokens <= 32767.  Reported log-probabilities stay the raw model distribution.
    # TP = 1 without CP only.
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    # the LoRA adapter the request runs on, by the name it was loaded under (LLMEngine.load_adapter);
    # None: the base model.  Rows of different adapters and of none share a step.  Llama at TP = 1
    # without CP only.
    adapter: Optional[str] = None


class SeqStatus(enum.Enum):
    WAITING = 0
    RUNNING = 1
    FINISHED = 2


_ids = itertools.count()


PENDING = -1   # placeholder token id (never fed to the model: gathered on the device instead)


class Sequence:
    def __init__(self, request_id: str, prompt_ids: List[int], params: SamplingParams, arrival: Optional[float] = None):
        self.seq_id = next(_ids)
        self.request_id = request_id
        self.prompt_ids = list(prompt_ids)
        self.output_ids: List[int] = []
        # with params.logprobs: one entry per EMITTED output token (every token a StepOutput has
        # handed out), so output_logprobs[i] belongs to output_ids[i] and the lists are equal in
        # length whenever nothing is in flight (always once finished); what output_ids holds beyond
        # -- a PENDING placeholder, a known run or a prompt-lookup draft of the step in flight -- has
        # no entry yet, so dropping a draft (drop_draft, a rejected verification) touches nothing
        # here.  A sampled token carries its log-probability, a token appended without a sample
        # (forced_output, jump-forward, grammar-forced) None.
        self.output_logprobs: List[Optional[float]] = []
        # with params.top_logprobs > 0: parallel to output_logprobs, by the same alignment rules -- a
        # sampled token carries its row's N (token id, log-probability) alternatives, a token appended
        # without a sample None.  The sampled token's output_logprobs entry comes from the same row of
        # logits: where the token is among its alternatives the two values are equal bit for bit.
        self.output_top_logprobs: List[Optional[List[Tuple[int, float]]]] = []
        self.params = params
        self.status = SeqStatus.WAITING
        self.block_table: List[int] = []
        self.num_computed = 0          # tokens whose KV is in the cache
        self.num_cached_prompt = 0     # prefix-cache hit (tokens)
        self.num_prefilled = 0         # tokens run through prefill chunks (recomputes included)
        self.arrival = time.perf_counter() if arrival is None else arrival
        self.first_token_time: Optional[float] = None
        self.admit_time: Optional[float] = None   # first admitted into a step (scheduler clock)
        self.finish_reason: Optional[str] = None
        self.seed = params.seed if params.seed is not None else (hash((request_id, self.seq_id)) & 0x7FFFFFFF)
        self.num_preemptions = 0
        # overlap scheduling (LLMEngine, async_scheduling): while step N runs, the sequence carries
        # a placeholder for N's sampled token (output_ids[-1] == PENDING); pending_src is its row in
        # N's sampled vector, gathered on the device by step N+1.  awaiting: N's token certainly
        # ends the sequence (length / forced end), so it sits out N+1.
        self.pending_src = -1
        self.awaiting = False
        self.jump_queue: List[int] = []    # grammar-forced tokens staged for the next launch
        self.last_run: List[int] = []      # tokens appended at launch (emitted on resolve)
        self.jump_tail: List[int] = []     # final run of an awaiting sequence
        # prompt-lookup speculation: spec_rows -- sampled positions at the tail of the next chunk
        # (draft + 1; 0 = an ordinary row); spec_reject -- draft tokens already known to be rejected
        # at launch (teacher-forced output) and dropped once the chunk is launched
        self.spec_rows = 0
        self.spec_reject = 0
        self.spec_lookup = None
        self.spec_proposed = 0
        self.spec_accepted = 0
        # constrained decoding: fsm_off -- offset of the request's automaton in the runner's device
        # tables (None: unconstrained); (fsm_pos, fsm_state) -- the host mirror: the automaton's local
        # state after the first fsm_pos output tokens (never past an unverified draft token)
        self.fsm_off: Optional[int] = None
        self.fsm_pos = 0
        self.fsm_state = 0
        # penalties: pen_slot -- the sequence's row of the runner's count table (-1: not penalised; kept
        # after the slot is released, whose contents stand until it is taken again); pen_held -- the
        # slot is this sequence's; pen_counted -- output tokens [0, pen_counted) are in the table
        self.pen_slot = -1
        self.pen_held = False
        self.pen_counted = 0
        # LoRA: lora_slot -- the adapter's slot of the engine's table (-1: the base model), carried by every
        # row of the sequence; cache_salt -- where the sequence's prefix-cache hash chain starts (0: the
        # base model; an adapter's salt, so its KV is shared with requests on the same load of it only)
        self.lora_slot = -1
        self.cache_salt = 0
        # host-memory KV tier (kv_host_tier): kv_discard -- nothing of the sequence is saved when its
        # blocks are freed (an abort); tier_wait -- a preempted sequence's admission is put off until
        # the pool can take it back whole from the tier, tier_waits -- how often that has happened
        self.kv_discard = False
        self.tier_wait = False
        self.tier_waits = 0

    def fsm_state_before(self, k: int) -> int:
        """Local automaton state in front of output token k (every earlier token known; -1: the
        output left the language, the row goes on unconstrained).  Advances the mirror over tokens
        that will not be taken back (a prompt-lookup draft in the tail may be)."""
        a = self.params.constraint
        if k < self.fsm_pos:
            self.fsm_pos, self.fsm_state = 0, a.start
        elif self.fsm_pos == 0:
            self.fsm_state = a.start
        stable = len(self.output_ids) - max(self.spec_rows - 1, 0)
        s = self.fsm_state
        out = self.output_ids
        for i in range(self.fsm_pos, k):
            s = a.advance(s, out[i])
            if i < stable:
                self.fsm_pos, self.fsm_state = i + 1, s
        return s

    def drop_draft(self) -> None:
        """Forget a prompt-lookup draft that was appended but never launched (preemption)."""
        m = self.spec_rows - 1
        if m > 0:
            accepted = m - self.spec_reject
            del self.output_ids[len(self.output_ids) - m:]
            if self.last_run and accepted:
                self.last_run = self.last_run[:len(self.last_run) - accepted]
        self.spec_rows = 0
        self.spec_reject = 0

    @property
    def priority_time(self) -> float:
        return self.arrival if self.params.priority_ts is None else self.params.priority_ts

    @property
    def all_ids(self) -> List[int]:
        return self.prompt_ids + self.output_ids

    def __len__(self) -> int:
        return len(self.prompt_ids) + len(self.output_ids)

    @property
    def num_tokens(self) -> int:
        return len(self)

    @property
    def in_prefill(self) -> bool:
        return self.num_computed < self.num_tokens - 1 or (self.num_computed == 0)

    @property
    def remaining_prefill(self) -> int:
        return self.num_tokens - self.num_computed

    @property
    def finished(self) -> bool:
        return self.status == SeqStatus.FINISHED

    def step_seed(self) -> int:
        """Per-token seed: depends only on the request and the position (batch-invariant)."""
        return self.step_seed_at(len(self.output_ids))

    def step_seed_at(self, k: int) -> int:
        """Seed of the sample that becomes output token k."""
        return (self.seed * 0x9E3779B1 + k * 0x85EBCA77 + 1) & 0x7FFFFFFFFFFFFFFF
