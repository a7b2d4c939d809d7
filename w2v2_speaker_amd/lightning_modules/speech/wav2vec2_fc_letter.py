"""Mirror of ref: src/lightning_modules/speech/wav2vec2_fc_letter.py (``Wav2vec2FcLetterRecognizer``) and of the step
semantics of ref: src/lightning_modules/speech/speech_recognition_module.py:91-248 on the HIP engine -- the experiment
config/experiment/speech_wav2vec2_ctc.yaml.  The wav2vec2 encoder, dropout + ``lm_head`` (a Linear onto the tokenizer's
vocabulary) on every frame, the CTC loss against the transcript, greedy decoding and the word error rate.

Like the speaker modules this is a ``torch.nn.Module`` with the reference's constructor arguments and method names, whose
``training_step`` runs forward, the hand-written backward and the fused optimiser itself (``automatic_optimization =
False``).  What differs from the reference's route: the logits never leave the device for the loss (three launches of
csrc/ctc_long.hip or csrc/ctc.hip, by the width of the batch's transcript tensor), and decoding is one launch and ONE
device-to-host copy per batch where the reference takes an argmax and synchronises per utterance.

Training batches differ in padded length, and a static plan is built per shape: the module keeps at most ``MAX_PLANS``
plans keyed by (batch, padded samples, kind), least recently used first out, each with its trainer.  The padded frames
of a batch run through the encoder as they do in the reference (``wav2vec2-base`` takes no attention mask); only the
loss and the decoder read the lengths.

``timestep_mask_prob`` / ``channel_mask_prob`` other than 0 raise: the reference's ``EmbeddingMasker`` draws from torch's
host RNG per step and is not built (the experiment's values are 0)."""
from __future__ import annotations

import warnings
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import torch

from ... import ops
from ...config import W2V2Config, Wav2Vec2RegularisationConfig
from ...data.speech import SpeechRecognitionDataBatch
from ...engine import Plan
from ...eval_batching import PlanCache
from ...evaluation.speech.wer import calculate_wer
from ...optim.loss import CtcLoss
from ...optim.schedule import OneCycle
from ...params import ParamStore
from ...tokenizer import BaseTokenizer, Wav2vec2Tokenizer
from ...trainer import SpeakerTrainer
from ..speaker._optim_surface import OptimizerSurface, prep_waveform_input
from ..speaker.wav2vec2_fc import Wav2vec2FCModule, _Wav2vecHandle, restore_from_checkpoint

MAX_PLANS = 6      # static plans (and their trainers) kept per module, least recently used first out
W_HEAD, B_HEAD = "speech_recognition_head.lm_head.weight", "speech_recognition_head.lm_head.bias"


@dataclass
class Wav2vec2FcLetterRecognizerConfig:
    """Same field names (and spelling) as ref: wav2vec2_fc_letter.py:30-58 / config/network/wav2vec2_fc_letter.yaml."""
    wav2vec_hunggingface_id: str = "facebook/wav2vec2-base"
    reset_weights: bool = False
    wav2vec_initially_frozen: bool = False
    completely_freeze_feature_extractor: bool = True
    num_frozen_steps: Optional[int] = 10000
    timestep_mask_prob: float = 0.0
    timestep_mask_width: int = 10
    channel_mask_prob: float = 0.0
    channel_mask_width: int = 64
    speech_head_huggingface_id: Optional[str] = None


class Wav2vec2FcLetterRecognizer(OptimizerSurface, torch.nn.Module):
    automatic_optimization = False

    def __init__(self, cfg: Wav2vec2FcLetterRecognizerConfig, hyperparameter_config, loss_fn_constructor: Callable[[], object],
                 tokenizer: BaseTokenizer, *, device="cuda", act_dtype: torch.dtype = torch.float16, max_lr: float = 1e-4,
                 max_steps: int = 100_000, process_group=None, init_seed: int = 20211, pretrained_state_dict=None,
                 gradient_clip_val: float = 0.0, accumulate_grad_batches: int = 1,
                 reg: Optional[Wav2Vec2RegularisationConfig] = None, final_dropout: float = 0.0,
                 max_target: int = ops.CTC_LONG_MAX_TARGET, train_wer_every: int = 100):
        """Positional arguments = ref: wav2vec2_fc_letter.py:90-96.  Keyword-only extras as in Wav2vec2FCModule, and:
        ``reg`` (the dropouts / LayerDrop / SpecAugment of the HF config the reference loads with the checkpoint),
        ``final_dropout`` (HF ``Wav2Vec2ForCTC.dropout``, 0 in ``facebook/wav2vec2-base``), ``max_target`` (the longest
        transcript a plan holds, at most 1023 letters) and ``train_wer_every`` (the training WER needs the decoded batch on
        the host: taken every that many steps, the reference's logging interval; 0 = never)."""
        super().__init__()
        self.gradient_clip_val = float(gradient_clip_val)
        self._set_accumulate_grad_batches(accumulate_grad_batches)
        self.hyperparameters_to_save = hyperparameter_config
        self.cfg = cfg
        loss_fn = loss_fn_constructor()
        if not isinstance(loss_fn, CtcLoss):      # ref: speech_recognition_module.py:47-50
            raise ValueError(f"expected loss class {CtcLoss}, got {loss_fn.__class__}")
        if int(loss_fn.blank_idx) != int(tokenizer.blank_token_id()):
            raise ValueError(f"CtcLoss(blank_idx={loss_fn.blank_idx}) but the tokenizer's blank is "
                             f"{tokenizer.blank_token_id()}")
        if cfg.timestep_mask_prob != 0 or cfg.channel_mask_prob != 0:
            raise NotImplementedError(f"timestep_mask_prob = {cfg.timestep_mask_prob}, channel_mask_prob = "
                                      f"{cfg.channel_mask_prob}: EmbeddingMasker (ref: src/layers/embedding_masking.py) "
                                      "is not built; config/experiment/speech_wav2vec2_ctc.yaml runs with 0 and 0")
        if (self.accumulate_grad_batches > 1 and cfg.wav2vec_initially_frozen and cfg.num_frozen_steps is not None
                and cfg.num_frozen_steps % self.accumulate_grad_batches != 0):
            raise ValueError(f"num_frozen_steps = {cfg.num_frozen_steps} is no multiple of accumulate_grad_batches = "
                             f"{self.accumulate_grad_batches}: the unfreeze would fall inside an accumulation window")
        if not 0.0 <= final_dropout < 1.0:
            raise ValueError(f"final_dropout = {final_dropout} outside [0, 1)")
        self.tokenizer = tokenizer
        self.vocab_size = int(tokenizer.vocabulary_size())
        self.blank = int(loss_fn.blank_idx)
        del loss_fn
        self.model_cfg = W2V2Config.from_huggingface_id(cfg.wav2vec_hunggingface_id)
        self.reg = reg if reg is not None else Wav2Vec2RegularisationConfig()
        self.final_dropout, self.max_target, self.train_wer_every = float(final_dropout), int(max_target), int(train_wer_every)
        self.store = ParamStore(self.model_cfg, device, act_dtype, head="letter", vocab_size=self.vocab_size,
                                freeze_cnn=cfg.completely_freeze_feature_extractor)
        self.store.init_weights(init_seed)
        if pretrained_state_dict is not None:
            sd = (torch.load(pretrained_state_dict, map_location="cpu", weights_only=True)
                  if isinstance(pretrained_state_dict, str) else pretrained_state_dict)
            self.store.load_state_dict(dict(sd), strict=False, prefix_model=True)
        elif not cfg.reset_weights:
            warnings.warn("Wav2vec2FcLetterRecognizer: reset_weights=False asks for the pretrained "
                          f"{cfg.wav2vec_hunggingface_id!r} weights, but none were given (pass pretrained_state_dict=): "
                          "the model starts from a RANDOM initialisation", stacklevel=2)
        # (what Wav2vec2FCModule.save_checkpoint records under hyper_parameters)
        self.loss, self.num_speakers = "letter", self.vocab_size
        self.schedule = OneCycle(max_lr=max_lr, total_steps=max_steps)
        self.process_group = process_group
        self._trainers: Dict[Tuple, SpeakerTrainer] = {}
        self._plans = PlanCache(MAX_PLANS, on_evict=lambda key: self._trainers.pop(key, None))
        self.steps = 0
        self.schedule_step = 0
        self._is_wav2vec_frozen = False
        self.device = torch.device(device)
        self.wav2vec = _Wav2vecHandle(self)
        self.train_wer: Optional[float] = None

    @classmethod
    def from_config(cls, cfg: Wav2vec2FcLetterRecognizerConfig, tokenizer: Optional[BaseTokenizer] = None,
                    **kw) -> "Wav2vec2FcLetterRecognizer":
        """Short form for scripts and tests: the packaged letter tokenizer and ``CtcLoss(long_targets=True)``."""
        tokenizer = tokenizer if tokenizer is not None else Wav2vec2Tokenizer()
        return cls(cfg, kw.pop("hyperparameter_config", None), lambda: CtcLoss(tokenizer.blank_token_id(), long_targets=True),
                   tokenizer, **kw)

    # ------------------------------------------------------------------ nn.Module surface over the flat arena
    def named_parameters(self, prefix: str = "", recurse: bool = True, remove_duplicate: bool = True):
        for n, p in self._parameter_views().items():
            yield (prefix + "." if prefix else "") + n, p

    def _apply(self, fn, recurse: bool = True):
        return self

    def _set_body_trainable(self, flag: bool) -> None:
        self._is_wav2vec_frozen = not flag

    def on_train_start(self) -> None:
        # ref: wav2vec2_fc_letter.py:177-185
        self.steps = 0
        if self.cfg.wav2vec_initially_frozen:
            self.wav2vec.freeze()
        if self.cfg.completely_freeze_feature_extractor:
            self.wav2vec.model.feature_extractor.requires_grad_(False)

    def on_after_backward(self) -> None:
        # ref: wav2vec2_fc_letter.py:187-199
        self.steps += 1
        if (self._is_wav2vec_frozen and self.cfg.num_frozen_steps is not None
                and self.steps >= self.cfg.num_frozen_steps):
            self.wav2vec.unfreeze()
            if self.cfg.completely_freeze_feature_extractor:
                self.wav2vec.model.feature_extractor.requires_grad_(False)

    # ------------------------------------------------------------------ plans
    @property
    def plans_built(self) -> int:
        return self._plans.built

    def _plan(self, batch: int, n: int, kind: str) -> Plan:
        """kind: "train", "frozen" (training head, eval-mode encoder) or "eval"."""
        noreg = Wav2Vec2RegularisationConfig(activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0,
                                             hidden_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0)
        return self._plans.lookup((batch, n, kind), lambda: Plan(
            self.store, batch, n, train=kind != "eval", reg=self.reg if kind == "train" else noreg, pooling="none",
            final_dropout=self.final_dropout if kind == "train" else 0.0, max_target=self.max_target))

    # ------------------------------------------------------------------ reference surface
    def _eval_forward(self, input_tensor: torch.Tensor, lengths: List[int]) -> Plan:
        x = prep_waveform_input(input_tensor).to(self.device, torch.float32)
        if len(lengths) != x.shape[0]:
            raise ValueError(f"{len(lengths)} lengths for a batch of {x.shape[0]}")
        plan = self._plan(x.shape[0], x.shape[1], "eval")
        plan.embed(x)
        return plan

    def compute_speech_embedding(self, input_tensor: torch.Tensor, lengths: List[int]):
        """ref: :124-149 -> ([B, T, H] embedding, the lengths in frames ``floor((n - 80) / 320)``)."""
        plan = self._eval_forward(input_tensor, lengths)
        return plan.emb.view(plan.B, plan.T, -1).clone(), plan.frames_of(lengths)

    def compute_vocabulary_prediction(self, embedding_tensor: torch.Tensor, lengths: List[int]):
        """ref: :151-157 -- the head on any [B, T, H] embedding (no dropout outside training); lengths pass through."""
        x = embedding_tensor.to(self.device, torch.float32)
        lead = x.shape[:-1]
        x = x.reshape(-1, x.shape[-1]).contiguous()
        out = torch.empty(x.shape[0], self.vocab_size, dtype=torch.float32, device=self.device)
        ops.skinny_linear_fwd(x, self.store.p(W_HEAD), self.store.p(B_HEAD), out, ops.ACT_NONE)
        return out.view(*lead, self.vocab_size), lengths

    def forward(self, input_tensor: torch.Tensor, lengths: List[int]):
        """ref: speech_recognition_module.py:91-98 -> ((embedding, frame lengths), (prediction, frame lengths)): one
        pass of the evaluation plan, the prediction is its head's logits."""
        plan = self._eval_forward(input_tensor, lengths)
        frames = plan.frames_of(lengths)
        plan.head.forward_only(frames)
        emb = plan.emb.view(plan.B, plan.T, -1).clone()
        pred = plan.head.logits[:, :self.vocab_size].reshape(plan.B, plan.T, self.vocab_size).clone()
        return (emb, frames), (pred, frames)

    def generate_example_input(self, include_batch_dimension: bool, batch_size: Optional[int] = None):
        shape = [batch_size, 16000] if include_batch_dimension else [16000]
        return torch.rand(size=shape), [16000]

    # ------------------------------------------------------------------ decoding
    def _decode_head(self, head) -> List[str]:
        tokens, counts = head.decoded()                # one launch, one copy to the host for the whole batch
        return self.tokenizer.decode_ids(tokens, counts)

    def _decode_letter_prediction(self, letter_prediction: torch.Tensor, lengths: List[int]) -> List[str]:
        """ref: speech_recognition_module.py:233-248 on any [B, T, V] prediction tensor."""
        z = letter_prediction.to(self.device, torch.float32).contiguous()
        B, T, V = z.shape
        il = torch.tensor([int(n) for n in lengths], dtype=torch.int32).to(self.device)
        dec = torch.zeros(B * T + B, dtype=torch.int32, device=self.device)
        ops.ctc_greedy_decode(z.view(B * T, V), il, dec[:B * T].view(B, T), dec[B * T:], B, T, V, V, blank=self.blank)
        host = dec.cpu()
        return self.tokenizer.decode_ids(host[:B * T].view(B, T), host[B * T:])

    # ------------------------------------------------------------------ steps
    @staticmethod
    def _transcript(batch: SpeechRecognitionDataBatch):
        gt = batch.ground_truth
        if gt.dim() == 1:
            gt = gt[None]
        return gt.to("cpu"), batch.ground_truth_sequence_length, [int(n) for n in batch.input_lengths]

    def training_step(self, batch: SpeechRecognitionDataBatch, batch_idx: int = 0, optimized_idx: Optional[int] = None):
        """ref: speech_recognition_module.py:100-146: forward + loss + backward + optimiser step; returns the loss (a
        device tensor, nothing waits for it).  ``self.train_wer``: the batch's WER every ``train_wer_every`` steps."""
        x = prep_waveform_input(batch.network_input).to(self.device, torch.float32)
        transcript = self._transcript(batch)
        kind = "frozen" if self._is_wav2vec_frozen else "train"
        key = (x.shape[0], x.shape[1], "train")
        plan = self._plan(x.shape[0], x.shape[1], "train")
        fplan = self._plan(x.shape[0], x.shape[1], "frozen") if kind == "frozen" else None

        def run(tr):
            if fplan is not None:
                return tr.train_step_frozen_encoder(fplan, x, None, transcript=transcript)
            return tr.train_step(x, None, transcript=transcript)

        loss, _ = self._trainer_step(
            key, lambda: SpeakerTrainer(self.store, plan, self.schedule, process_group=self.process_group,
                                        **self._trainer_options()), run)
        self.on_after_backward()
        if self.train_wer_every > 0 and batch_idx % self.train_wer_every == 0:
            self.train_wer = calculate_wer(self._decode_head((fplan or plan).head), batch.ground_truth_strings)
        return loss

    def _eval_step(self, batch: SpeechRecognitionDataBatch, with_loss: bool):
        plan = self._eval_forward(batch.network_input, batch.input_lengths)
        loss = None
        if with_loss:
            loss, _ = plan.head_forward_backward(None, transcript=self._transcript(batch))
        else:
            plan.head.forward_only(plan.frames_of(batch.input_lengths))
        return loss, self._decode_head(plan.head)

    def validation_step(self, batch: SpeechRecognitionDataBatch, batch_idx: int = 0, dataloader_idx: Optional[int] = None):
        loss, transcription = self._eval_step(batch, True)
        return {"val_loss": loss, "transcription": transcription, "ground_truth": batch.ground_truth_strings}

    def test_step(self, batch: SpeechRecognitionDataBatch, batch_idx: int = 0, dataloader_idx: Optional[int] = None):
        _, transcription = self._eval_step(batch, False)
        return {"transcription": transcription, "ground_truth": batch.ground_truth_strings}

    @staticmethod
    def _calculate_wer_on_collected_output(output: List[dict]) -> float:
        transcriptions, ground_truths = [], []
        for d in output:
            transcriptions.extend(d["transcription"])
            ground_truths.extend(d["ground_truth"])
        return calculate_wer(transcriptions, ground_truths)

    def validation_epoch_end(self, outputs: List[List[dict]]) -> dict:
        """ref: :178-193 -- ``outputs``: one list per dataloader (LibriSpeech dev-clean, dev-other)."""
        out = {}
        for name, o in zip(("clean", "other"), outputs):
            out[f"val_loss_{name}"] = float(torch.stack([torch.as_tensor(d["val_loss"]).float().cpu() for d in o]).mean())
            out[f"val_wer_{name}"] = self._calculate_wer_on_collected_output(o)
        return out

    def test_epoch_end(self, outputs: List[List[dict]]) -> dict:
        return {f"test_wer_{name}": self._calculate_wer_on_collected_output(o) for name, o in zip(("clean", "other"), outputs)}

    # ------------------------------------------------------------------ checkpoints (reference key names)
    def state_dict(self, *args, **kwargs):
        return self.store.state_dict()

    def load_state_dict(self, sd, strict: bool = True, assign: bool = False):
        self.store.load_state_dict(sd, strict=strict, prefix_model=False)

    # the PL-1.4-style file of the speaker module, written and read by the same code: it touches the store, the schedule
    # and the counters this class names the same way (state_dict keys: ``wav2vec.model.*``,
    # ``speech_recognition_head.lm_head.*``)
    save_checkpoint = Wav2vec2FCModule.save_checkpoint

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path: str, strict: bool = False, **kwargs) -> "Wav2vec2FcLetterRecognizer":
        kwargs.setdefault("hyperparameter_config", None)
        return restore_from_checkpoint(cls, checkpoint_path, strict, kwargs)
