"""Local inference engine: tokenizer, chat template, paged KV + prefix cache, continuous
batching scheduler, model runner with hipGraph decode, async front-end."""
from .kv_calibration import calibrate_kv_scales, save_kv_scales
from .llm_engine import LLMEngine, ScoreResult, StepOutput
from .sequence import SamplingParams, Sequence

__all__ = ["LLMEngine", "ScoreResult", "StepOutput", "SamplingParams", "Sequence",
           "calibrate_kv_scales", "save_kv_scales"]
