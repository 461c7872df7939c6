//! `impl Processor` for the HIP-backed Scale / Model / ColorCode.
//!
//! UNTESTED: never compiled (no Rust toolchain in the build environment).  Written against the
//! reference's trait (`infur/src/processing.rs:23-60`); inside the `infur` crate replace
//! `use crate::processing::Processor` accordingly and swap the three type names in
//! `ProcessingApp` (`infur/src/app.rs:51-62`).
use std::{ffi::{CStr, CString}, rc::Rc};

use eframe::epaint::{Color32, ColorImage};
use image_ext::BgrImage;
use infur_hip_sys as sys;
use ndarray::{Array3, ArrayD, IxDyn};
use thiserror::Error;

/// The reference's plugin contract, restated so this crate stands alone.
pub trait Processor {
    type Command;
    type ControlError;
    type Input;
    type Output;
    type ProcessResult;
    fn control(&mut self, cmd: Self::Command) -> Result<&mut Self, Self::ControlError>;
    fn advance(&mut self, inp: &Self::Input, out: &mut Self::Output) -> Self::ProcessResult;
    fn is_dirty(&self) -> bool;
    /// Provided method of the reference's trait (`infur/src/processing.rs:53-59`): run the node on default input and
    /// output -- how the `Proc` loop drives the final node of the graph (`main.rs:85`).
    fn generate(&mut self) -> Self::ProcessResult
    where
        Self::Input: Default,
        Self::Output: Default,
    {
        let inp = <Self::Input as Default>::default();
        let mut out = <Self::Output as Default>::default();
        self.advance(&inp, &mut out)
    }
}

pub struct Frame {
    pub id: u64,
    pub img: BgrImage,
}

/// One GPU + one HIP stream.  `!Send`: keep it on the `Proc` thread like the ORT session
/// (`infur/src/main.rs:38-40`).
pub struct Ctx(*mut sys::infur_ctx);

impl Ctx {
    pub fn new(device: i32) -> Result<Rc<Self>, HipError> {
        let mut o = std::mem::MaybeUninit::<sys::infur_options>::uninit();
        let mut ctx = std::ptr::null_mut();
        let rc = unsafe {
            sys::infur_options_default(o.as_mut_ptr());
            let mut o = o.assume_init();
            o.device = device;
            sys::infur_ctx_create(&o, &mut ctx)
        };
        if rc != sys::INFUR_OK { return Err(HipError::status(rc)); }
        Ok(Rc::new(Ctx(ctx)))
    }
    fn err(&self, rc: i32) -> HipError {
        let msg = unsafe { CStr::from_ptr(sys::infur_last_error(self.0)) }.to_string_lossy().into_owned();
        HipError { code: rc, msg }
    }
    /// the decisions of the tile-configuration tuner so far, as text (`infur_tune_export`): feed it to `tuning_import` of a later
    /// process and its first frame finds every conv shape's configuration already measured
    pub fn tuning_text(&self) -> Result<String, HipError> {
        let mut len = 0usize;
        let rc = unsafe { sys::infur_tune_export(self.0, std::ptr::null_mut(), 0, &mut len) };
        if rc != sys::INFUR_OK { return Err(self.err(rc)); }
        let mut buf = vec![0u8; len + 1];
        let rc = unsafe { sys::infur_tune_export(self.0, buf.as_mut_ptr() as *mut std::os::raw::c_char, buf.len(), &mut len) };
        if rc != sys::INFUR_OK { return Err(self.err(rc)); }
        buf.truncate(len);
        Ok(String::from_utf8_lossy(&buf).into_owned())
    }
    pub fn tuning_import(&self, text: &str) -> Result<(), HipError> {
        let rc = unsafe { sys::infur_tune_import(self.0, text.as_ptr() as *const std::os::raw::c_char, text.len()) };
        if rc != sys::INFUR_OK { return Err(self.err(rc)); }
        Ok(())
    }
    /// per-kernel HIP-event records of the last advance (after `set_profile(true)`): (layer, kernel family, milliseconds, FLOPs, bytes)
    pub fn set_profile(&self, on: bool) -> Result<(), HipError> {
        let rc = unsafe { sys::infur_profile_enable(self.0, on as u32) };
        if rc != sys::INFUR_OK { return Err(self.err(rc)); }
        Ok(())
    }
    /// INFUR_DTYPE_F16_HL contexts: the opt-in range monitor (`infur_hl_monitor_enable`; an error in the other modes)
    pub fn set_hl_monitor(&self, on: bool) -> Result<(), HipError> {
        let rc = unsafe { sys::infur_hl_monitor_enable(self.0, on as u32) };
        if rc != sys::INFUR_OK { return Err(self.err(rc)); }
        Ok(())
    }
    /// what the monitor saw since it was enabled or last read, and clears it (`infur_hl_range`): (max |activation|, max |Winograd-domain
    /// input|, saturated, NaN seen).  A saturated frame is not f16hl-grade: re-run it on an f32 / f32-split context
    pub fn hl_range(&self) -> Result<(f32, f32, bool, bool), HipError> {
        let (mut act, mut wino, mut sat, mut nan) = (0f32, 0f32, 0u32, 0u32);
        let rc = unsafe { sys::infur_hl_range(self.0, &mut act, &mut wino, &mut sat, &mut nan) };
        if rc != sys::INFUR_OK { return Err(self.err(rc)); }
        Ok((act, wino, sat != 0, nan != 0))
    }
    pub fn profile(&self) -> Result<Vec<(String, String, f32, f64, f64)>, HipError> {
        let mut n = 0u32;
        let rc = unsafe { sys::infur_profile_count(self.0, &mut n) };
        if rc != sys::INFUR_OK { return Err(self.err(rc)); }
        let mut out = Vec::with_capacity(n as usize);
        for i in 0..n {
            let mut rec = std::mem::MaybeUninit::<sys::infur_kernel_record>::zeroed();
            let rc = unsafe { sys::infur_profile_get(self.0, i, rec.as_mut_ptr()) };
            if rc != sys::INFUR_OK { return Err(self.err(rc)); }
            let rec = unsafe { rec.assume_init() };
            let name = unsafe { CStr::from_ptr(rec.name.as_ptr()) }.to_string_lossy().into_owned();
            let kernel = unsafe { CStr::from_ptr(rec.kernel.as_ptr()) }.to_string_lossy().into_owned();
            out.push((name, kernel, rec.ms, rec.flops, rec.bytes));
        }
        Ok(out)
    }
}
impl Drop for Ctx {
    fn drop(&mut self) { unsafe { sys::infur_ctx_destroy(self.0) } }
}

#[derive(Error, Debug)]
#[error("{msg} (status {code})")]
pub struct HipError { pub code: i32, pub msg: String }
impl HipError {
    fn status(rc: i32) -> Self {
        let msg = unsafe { CStr::from_ptr(sys::infur_status_string(rc)) }.to_string_lossy().into_owned();
        HipError { code: rc, msg }
    }
    /// the context's own message for `rc` (infur_last_error), falling back to the status string
    fn from_ctx(ctx: &Ctx, rc: i32) -> Self {
        let p = unsafe { sys::infur_last_error(ctx.0) };
        if p.is_null() { return Self::status(rc); }
        let msg = unsafe { CStr::from_ptr(p) }.to_string_lossy().into_owned();
        if msg.is_empty() { Self::status(rc) } else { HipError { code: rc, msg } }
    }
}

// ---------------------------------------------------------------- Scale (processing.rs:142-282)
#[derive(PartialEq, Debug, Clone, Copy)]
pub struct ValidScale(f32);
#[derive(Error, Debug)]
#[error("Cannot scale by negative number")]
pub struct ValidScaleError;
impl TryFrom<f32> for ValidScale {
    type Error = ValidScaleError;
    fn try_from(v: f32) -> Result<Self, Self::Error> {
        if unsafe { sys::infur_scale_validate(v) } != sys::INFUR_OK { Err(ValidScaleError) } else { Ok(Self(v)) }
    }
}

#[derive(Error, Debug)]
pub enum ScaleProcError {
    #[error("scaling from 0-sized input")]
    ZeroSizeIn,
    #[error("scaling to 0-sized output")]
    ZeroSizeOut,
    #[error(transparent)]
    Hip(#[from] HipError),
}

pub struct HipScale { ctx: Rc<Ctx>, factor: ValidScale, dirty: bool, mode: u32 }
impl HipScale {
    pub fn new(ctx: Rc<Ctx>) -> Self { Self { ctx, factor: ValidScale(1.0), dirty: true, mode: sys::INFUR_SCALE_NEAREST } }
}
impl Processor for HipScale {
    type Command = f32;
    type ControlError = ValidScaleError;
    type Input = Option<Frame>;
    type Output = Option<Frame>;
    type ProcessResult = Result<(), ScaleProcError>;

    fn control(&mut self, cmd: f32) -> Result<&mut Self, ValidScaleError> {
        let factor: ValidScale = cmd.try_into()?;
        self.dirty = factor != self.factor;
        self.factor = factor;
        Ok(self)
    }
    fn is_dirty(&self) -> bool { self.dirty }
    fn advance(&mut self, input: &Option<Frame>, out: &mut Option<Frame>) -> Result<(), ScaleProcError> {
        self.dirty = false;
        let input = match input { Some(i) => i, None => return Ok(()) };
        if self.factor.0 == 1.0 {
            *out = Some(Frame { id: input.id, img: input.img.clone() });
            return Ok(());
        }
        let (w, h) = (input.img.width(), input.img.height());
        let (mut ow, mut oh) = (0u32, 0u32);
        match unsafe { sys::infur_scale_out_dims(w, h, self.factor.0, &mut ow, &mut oh) } {
            sys::INFUR_E_ZERO_SIZE_IN => return Err(ScaleProcError::ZeroSizeIn),
            sys::INFUR_E_ZERO_SIZE_OUT => return Err(ScaleProcError::ZeroSizeOut),
            _ => {}
        }
        let frame = out.get_or_insert_with(|| Frame { id: input.id, img: BgrImage::new(ow, oh) });
        if frame.img.width() != ow || frame.img.height() != oh { frame.img = BgrImage::new(ow, oh); }
        frame.id = input.id;
        let cap = frame.img.as_raw().len();
        let rc = unsafe {
            sys::infur_scale(self.ctx.0, input.img.as_raw().as_ptr(), w, h, self.factor.0, self.mode,
                             frame.img.as_mut().as_mut_ptr(), cap, &mut ow, &mut oh)
        };
        if rc == sys::INFUR_OK { Ok(()) } else { Err(self.ctx.err(rc).into()) }
    }
}

// ---------------------------------------------------------------- Model (predict_onnx.rs:146-345)
#[derive(Clone, Debug)]
pub enum ModelCmd { Load(String) }
#[derive(Debug, Clone)]
pub struct ModelInfo { pub input_names: Vec<String>, pub input0_dtype: String, pub output_names: Vec<String>, pub quantised: bool, pub resize_u8_heads: bool }

pub struct HipModel { ctx: Rc<Ctx> }
impl HipModel {
    pub fn new(ctx: Rc<Ctx>) -> Self { Self { ctx } }
    fn raw_info(&self) -> Option<sys::infur_model_info> {
        let mut mi = std::mem::MaybeUninit::<sys::infur_model_info>::uninit();
        if unsafe { sys::infur_model_info_get(self.ctx.0, mi.as_mut_ptr()) } != sys::INFUR_OK { return None; }
        Some(unsafe { mi.assume_init() })
    }
    pub fn get_info(&self) -> Option<ModelInfo> {
        let mi = self.raw_info()?;
        let s = |p: *const std::os::raw::c_char| unsafe { CStr::from_ptr(p) }.to_string_lossy().into_owned();
        Some(ModelInfo {
            input_names: vec![s(mi.input_name.as_ptr())],
            input0_dtype: s(mi.input0_dtype.as_ptr()),
            output_names: (0..mi.n_outputs as usize).map(|i| s(mi.output_names[i].as_ptr())).collect(),
            quantised: mi.quantised != 0,
            resize_u8_heads: mi.resize_u8_heads != 0,
        })
    }
}
/// Error processing model -- the reference's `ModelProcError` (`predict_onnx.rs:32-39`) with the ORT arm replaced
/// by the HIP runtime's (same variant names, same messages, so `AppProcError` keeps its `#[from]`, app.rs:17-36)
#[derive(Error, Debug)]
pub enum ModelProcError {
    #[error("couldn't transform image")]
    ShapeError(#[from] ndarray::ShapeError),
    #[error("scaling to 0-sized output")]
    RuntimeError(#[from] HipError),
}

/// Error loading model -- the reference's `ModelCmdError` (`predict_onnx.rs:41-48`): the runtime's own load error,
/// or the file's input 0 not being an image the path can run (`infer_img_pre_proc`, `predict_onnx.rs:223-265`)
#[derive(Error, Debug)]
pub enum ModelCmdError {
    #[error(transparent)]
    Hip(HipError),
    #[error(transparent)]
    RuntimeError(#[from] ModelInputFormatError),
}

#[derive(Error, Debug)]
pub enum ModelInputFormatError {
    #[error("couldn't infer image input")]
    Infer(String),
}

impl Processor for HipModel {
    type Command = ModelCmd;
    type ControlError = ModelCmdError;
    type Input = BgrImage;
    type Output = Vec<ArrayD<f32>>;
    type ProcessResult = Result<(), ModelProcError>;

    fn control(&mut self, cmd: ModelCmd) -> Result<&mut Self, ModelCmdError> {
        let ModelCmd::Load(path) = cmd; // "" unloads inside the library (predict_onnx.rs:310-312)
        let c = CString::new(path).map_err(|_| ModelCmdError::Hip(HipError { code: sys::INFUR_E_INVALID_ARG, msg: "path contains NUL".into() }))?;
        match unsafe { sys::infur_model_load(self.ctx.0, c.as_ptr()) } {
            sys::INFUR_OK => Ok(self),
            // the library reports input-layout problems with the reference's own messages (onnx_reader.cpp)
            sys::INFUR_E_MODEL_FORMAT => Err(ModelInputFormatError::Infer(self.ctx.err(sys::INFUR_E_MODEL_FORMAT).msg).into()),
            rc => Err(ModelCmdError::Hip(self.ctx.err(rc))),
        }
    }
    fn is_dirty(&self) -> bool { false }
    fn advance(&mut self, img: &BgrImage, out: &mut Vec<ArrayD<f32>>) -> Result<(), ModelProcError> {
        let mi = match self.raw_info() { Some(mi) => mi, None => return Ok(()) }; // no session: out untouched
        let (k, h, w) = (mi.num_classes as usize, img.height() as usize, img.width() as usize);
        // as many tensors as the model has outputs: [out, aux], or [out] without the aux head
        let mut bufs: Vec<Vec<f32>> = (0..mi.n_outputs).map(|_| vec![0f32; k * h * w]).collect();
        let aux = if bufs.len() > 1 { bufs[1].as_mut_ptr() } else { std::ptr::null_mut() };
        let mut n = 0u32;
        let rc = unsafe {
            sys::infur_model_advance(self.ctx.0, img.as_raw().as_ptr(), w as u32, h as u32,
                                     bufs[0].as_mut_ptr(), aux, &mut n)
        };
        if rc != sys::INFUR_OK { return Err(self.ctx.err(rc).into()); }
        out.clear();
        for b in bufs { out.push(ArrayD::from_shape_vec(IxDyn(&[k, h, w]), b)?); }
        Ok(())
    }
}

// ---------------------------------------------------------------- several GPUs (main.rs:38-40: one Proc thread)
/// `infur_group`: the contexts of one process driven together -- RCCL weight broadcast over xGMI and frame-batch
/// sharding (BASELINE configs[3]).  The `Ctx`s are kept alive by the `Rc`s held here.
pub struct HipGroup { raw: *mut sys::infur_group, ctxs: Vec<Rc<Ctx>> }
impl HipGroup {
    pub fn new(ctxs: Vec<Rc<Ctx>>) -> Result<Self, HipError> {
        let ptrs: Vec<*mut sys::infur_ctx> = ctxs.iter().map(|c| c.0).collect();
        let mut raw = std::ptr::null_mut();
        match unsafe { sys::infur_group_create(ptrs.as_ptr(), ptrs.len() as u32, &mut raw) } {
            sys::INFUR_OK => Ok(Self { raw, ctxs }),
            rc => Err(ctxs[0].err(rc)),
        }
    }
    fn err(&self, rc: i32) -> HipError {
        let msg = unsafe { CStr::from_ptr(sys::infur_group_last_error(self.raw)) }.to_string_lossy().into_owned();
        HipError { code: rc, msg }
    }
    /// Replicate the model loaded in `ctxs[root]` to every other context (one ncclBroadcast of the repacked arena).
    pub fn weights_broadcast(&mut self, root: u32) -> Result<(), HipError> {
        match unsafe { sys::infur_group_weights_broadcast(self.raw, root) } { sys::INFUR_OK => Ok(()), rc => Err(self.err(rc)) }
    }
    /// scale -> model -> decode for a batch of independent frames, contiguous slices per context, masks in frame order.
    pub fn batch_advance(&mut self, frames: &[BgrImage], factor: f32, masks: &mut Vec<ColorImage>) -> Result<(), HipError> {
        masks.clear();
        for f in frames {
            let (mut ow, mut oh) = (0u32, 0u32);
            let rc = unsafe { sys::infur_scale_out_dims(f.width(), f.height(), factor, &mut ow, &mut oh) };
            if rc != sys::INFUR_OK { return Err(HipError::status(rc)); }
            masks.push(ColorImage::new([ow as usize, oh as usize], Color32::BLACK));
        }
        let ins: Vec<*const u8> = frames.iter().map(|f| f.as_raw().as_ptr()).collect();
        let outs: Vec<*mut u8> = masks.iter_mut().map(|m| m.pixels.as_mut_ptr() as *mut u8).collect();
        let ws: Vec<u32> = frames.iter().map(|f| f.width()).collect();
        let hs: Vec<u32> = frames.iter().map(|f| f.height()).collect();
        let caps: Vec<usize> = masks.iter().map(|m| m.pixels.len() * 4).collect();
        let rc = unsafe {
            sys::infur_group_batch_advance(self.raw, ins.as_ptr(), ws.as_ptr(), hs.as_ptr(), frames.len() as u32, factor,
                                           sys::INFUR_SCALE_NEAREST, outs.as_ptr(), caps.as_ptr(), std::ptr::null_mut(), std::ptr::null_mut())
        };
        if rc == sys::INFUR_OK { Ok(()) } else { Err(self.err(rc)) }
    }
    pub fn len(&self) -> usize { self.ctxs.len() }
}
impl Drop for HipGroup {
    fn drop(&mut self) { unsafe { sys::infur_group_destroy(self.raw) } }
}

// ---------------------------------------------------------------- ColorCode (decode_predict.rs:38-84)
pub struct HipColorCode { ctx: Rc<Ctx> }
impl HipColorCode { pub fn new(ctx: Rc<Ctx>) -> Self { Self { ctx } } }
impl Processor for HipColorCode {
    type Command = ();
    type ControlError = ();
    type Input = Array3<f32>;
    type Output = Option<ColorImage>;
    type ProcessResult = ();

    fn control(&mut self, _cmd: ()) -> Result<&mut Self, ()> { Ok(self) }
    fn is_dirty(&self) -> bool { false }
    fn advance(&mut self, inp: &Array3<f32>, out: &mut Option<ColorImage>) {
        let s = inp.shape();
        let (k, h, w) = (s[0], s[1], s[2]);
        let img = out.get_or_insert_with(|| ColorImage::new([w, h], Color32::BLACK));
        if img.width() != w || img.height() != h { *img = ColorImage::new([w, h], Color32::BLACK); }
        let std = inp.as_standard_layout();
        // Color32 is #[repr(C)] [u8; 4] premultiplied r,g,b,a: exactly the bytes the kernel writes
        unsafe {
            sys::infur_colorcode(self.ctx.0, std.as_ptr(), k as u32, h as u32, w as u32,
                                 img.pixels.as_mut_ptr() as *mut u8);
        }
    }
}

// ---------------------------------------------------------------- Segments (ColorCode's sibling for a headless host)
/// What `HipSegments` produces.  `klass` / `conf` are `h * w` bytes, `stats` is `classes` rows of `INFUR_STAT_WORDS` words (index
/// with `sys::INFUR_STAT_*`), `rgba` the overlay shaded by `conf`.  The `want_*` flags select the outputs; the others stay empty.
pub struct Segments {
    pub want_klass: bool, pub want_conf: bool, pub want_stats: bool, pub want_rgba: bool,
    pub size: [usize; 2], pub classes: usize,
    pub klass: Vec<u8>, pub conf: Vec<u8>, pub stats: Vec<u64>, pub rgba: Vec<u8>,
}
impl Default for Segments {
    fn default() -> Self {
        Self { want_klass: true, want_conf: true, want_stats: true, want_rgba: false, size: [0, 0], classes: 0,
               klass: Vec::new(), conf: Vec::new(), stats: Vec::new(), rgba: Vec::new() }
    }
}
impl Segments {
    pub fn stat(&self, k: usize, word: u32) -> u64 { self.stats[k * sys::INFUR_STAT_WORDS as usize + word as usize] }
}
/// Per-pixel argmax class, confidence byte, per-class statistics, optionally the shaded overlay.  Command = decode mode:
/// `INFUR_DECODE_RAW` is the loop of decode_predict.rs:67-78, `INFUR_DECODE_SOFTMAX` the same loop over logits with the softmax
/// probability of the winner as confidence (the README's "softmax if model predictions are logits").
pub struct HipSegments { ctx: Rc<Ctx>, decode: u32, dirty: bool }
impl HipSegments { pub fn new(ctx: Rc<Ctx>) -> Self { Self { ctx, decode: sys::INFUR_DECODE_RAW, dirty: true } } }
impl Processor for HipSegments {
    type Command = u32;
    type ControlError = HipError;
    type Input = Array3<f32>;
    type Output = Segments;
    type ProcessResult = Result<(), HipError>;

    fn control(&mut self, cmd: u32) -> Result<&mut Self, HipError> {
        if cmd > sys::INFUR_DECODE_SOFTMAX { return Err(HipError::status(sys::INFUR_E_INVALID_ARG)); } // state untouched
        self.dirty = cmd != self.decode;
        self.decode = cmd;
        Ok(self)
    }
    fn is_dirty(&self) -> bool { self.dirty }
    fn advance(&mut self, inp: &Array3<f32>, out: &mut Segments) -> Result<(), HipError> {
        self.dirty = false;
        let s = inp.shape();
        let (k, h, w) = (s[0], s[1], s[2]);
        out.size = [w, h];
        out.classes = k;
        out.klass.resize(if out.want_klass { h * w } else { 0 }, 0);
        out.conf.resize(if out.want_conf { h * w } else { 0 }, 0);
        out.stats.resize(if out.want_stats { k * sys::INFUR_STAT_WORDS as usize } else { 0 }, 0);
        out.rgba.resize(if out.want_rgba { h * w * 4 } else { 0 }, 0);
        fn ptr<T>(want: bool, v: &mut Vec<T>) -> *mut T { if want { v.as_mut_ptr() } else { std::ptr::null_mut() } }
        let std = inp.as_standard_layout();
        let rc = unsafe {
            sys::infur_segments(self.ctx.0, std.as_ptr(), k as u32, h as u32, w as u32, self.decode, ptr(out.want_klass, &mut out.klass),
                                ptr(out.want_conf, &mut out.conf), ptr(out.want_stats, &mut out.stats), ptr(out.want_rgba, &mut out.rgba))
        };
        if rc == sys::INFUR_OK { Ok(()) } else { Err(HipError::from_ctx(&self.ctx, rc)) }
    }
}

// ---------------------------------------------------------------- Regions (connected components of the class plane)
/// What `HipRegions` consumes: the planes `HipSegments` wrote (`conf` may be empty: the rows' SUM_CONF is then 0).
#[derive(Default)]
pub struct Planes { pub size: [usize; 2], pub klass: Vec<u8>, pub conf: Vec<u8> }
/// What `HipRegions` produces.  `labels` is `h * w` region ids (`sys::INFUR_REGION_NONE`: no kept region), `table` holds
/// `min(n, table_rows)` rows of `INFUR_REGION_WORDS` words in ascending order of the regions' first pixel, `n` counts every kept region.
pub struct Regions {
    pub want_labels: bool, pub table_rows: usize,
    pub size: [usize; 2], pub n: u32,
    pub labels: Vec<u32>, pub table: Vec<u64>,
}
impl Default for Regions {
    fn default() -> Self { Self { want_labels: true, table_rows: 1024, size: [0, 0], n: 0, labels: Vec::new(), table: Vec::new() } }
}
impl Regions {
    pub fn rows(&self) -> usize { (self.n as usize).min(self.table_rows) }
    pub fn word(&self, id: usize, word: u32) -> u64 { self.table[id * sys::INFUR_REGION_WORDS as usize + word as usize] }
}
pub enum RegionsCmd { Connectivity(u32), MinPixels(u32), Flags(u32) }
/// Connected components of the class plane under 4- or 8-connectivity, speckle below `min_pixels` dropped, optionally without the
/// background class.  Integer results, identical from run to run.
pub struct HipRegions { ctx: Rc<Ctx>, connectivity: u32, min_pixels: u32, flags: u32, dirty: bool }
impl HipRegions {
    pub fn new(ctx: Rc<Ctx>) -> Self { Self { ctx, connectivity: sys::INFUR_CONNECT_8, min_pixels: 0, flags: 0, dirty: true } }
}
impl Processor for HipRegions {
    type Command = RegionsCmd;
    type ControlError = HipError;
    type Input = Planes;
    type Output = Regions;
    type ProcessResult = Result<(), HipError>;

    fn control(&mut self, cmd: RegionsCmd) -> Result<&mut Self, HipError> {
        match cmd {  // a refused command leaves the state untouched
            RegionsCmd::Connectivity(v) => {
                if v != sys::INFUR_CONNECT_4 && v != sys::INFUR_CONNECT_8 { return Err(HipError::status(sys::INFUR_E_INVALID_ARG)); }
                self.dirty |= v != self.connectivity;
                self.connectivity = v;
            }
            RegionsCmd::MinPixels(v) => { self.dirty |= v != self.min_pixels; self.min_pixels = v; }
            RegionsCmd::Flags(v) => {
                if v & !sys::INFUR_REGIONS_SKIP_BACKGROUND != 0 { return Err(HipError::status(sys::INFUR_E_INVALID_ARG)); }
                self.dirty |= v != self.flags;
                self.flags = v;
            }
        }
        Ok(self)
    }
    fn is_dirty(&self) -> bool { self.dirty }
    fn advance(&mut self, inp: &Planes, out: &mut Regions) -> Result<(), HipError> {
        self.dirty = false;
        let [w, h] = inp.size;
        if inp.klass.len() != w * h || (!inp.conf.is_empty() && inp.conf.len() != w * h) { return Err(HipError::status(sys::INFUR_E_SHAPE)); }
        out.size = inp.size;
        out.labels.resize(if out.want_labels { h * w } else { 0 }, sys::INFUR_REGION_NONE);
        out.table.resize(out.table_rows * sys::INFUR_REGION_WORDS as usize, 0);
        let rc = unsafe {
            sys::infur_regions(self.ctx.0, inp.klass.as_ptr(), if inp.conf.is_empty() { std::ptr::null() } else { inp.conf.as_ptr() },
                               h as u32, w as u32, self.connectivity, self.min_pixels, self.flags,
                               if out.want_labels { out.labels.as_mut_ptr() } else { std::ptr::null_mut() },
                               if out.table_rows > 0 { out.table.as_mut_ptr() } else { std::ptr::null_mut() }, out.table_rows as u32, &mut out.n)
        };
        if rc == sys::INFUR_OK { Ok(()) } else { Err(HipError::from_ctx(&self.ctx, rc)) }
    }
}

// ---------------------------------------------------------------- Tracks (region identities from frame to frame)
/// What `HipTracks` produces: `track_of_region` and `table` (rows of `INFUR_TRACK_WORDS` words) hold one entry per region row of
/// the input, in region order (`sys::INFUR_TRACK_NONE`: not tracked); `plane` is `h * w` track ids; `summary` the four
/// `INFUR_TRACKS_SUMMARY_*` words.
#[derive(Default)]
pub struct Tracks {
    pub want_plane: bool, pub rows: usize,
    pub track_of_region: Vec<u32>, pub plane: Vec<u32>, pub table: Vec<u64>, pub summary: [u32; 4],
}
impl Tracks {
    pub fn status(&self) -> u32 { self.summary[sys::INFUR_TRACKS_SUMMARY_STATUS as usize] }
    pub fn word(&self, id: usize, word: u32) -> u64 { self.table[id * sys::INFUR_TRACK_WORDS as usize + word as usize] }
}
pub enum TracksCmd { MinOverlap(u32), Reset(u32) }
/// Owns one tracker (`infur_tracker_*`): the frame it remembers lives on the device.  A region inherits the track of the remembered
/// region of its class it overlaps most (when that region prefers it too), otherwise it starts a new one.  Integer results.
pub struct HipTracks { raw: *mut std::ffi::c_void, ctx: Rc<Ctx>, min_overlap: u32, dirty: bool }
impl HipTracks {
    /// `max_regions` / `pair_slots`: 0 = the library's defaults (65536, 1 << 20)
    pub fn new(ctx: Rc<Ctx>, max_regions: u32, pair_slots: u32) -> Result<Self, HipError> {
        let mut raw = std::ptr::null_mut();
        let rc = unsafe { sys::infur_tracker_create(ctx.0, max_regions, pair_slots, &mut raw) };
        if rc != sys::INFUR_OK { return Err(HipError::from_ctx(&ctx, rc)); }
        Ok(Self { raw, ctx, min_overlap: 1, dirty: true })
    }
    /// Keep lost tracks for up to `max_lost` steps (0: memory off, the other two are ignored): a region that would start a new track
    /// takes a lost track of its class back when its box meets that track's last box grown by `reach` pixels per step of absence.
    /// `gallery_rows`: 0 = 4096, at most 65536.  Forgets the remembered frame and the gallery.
    pub fn set_memory(&mut self, max_lost: u32, reach: u32, gallery_rows: u32) -> Result<(), HipError> {
        let rc = unsafe { sys::infur_tracker_set_memory(self.raw, max_lost, reach, gallery_rows) };
        if rc != sys::INFUR_OK { return Err(HipError::from_ctx(&self.ctx, rc)); }
        self.dirty = true;
        Ok(())
    }
    /// What the last step left on a tracker with memory: `rows` words of gap_of_region, the four `INFUR_TRACK_MEMORY_*` words and
    /// the first `min(HELD, lost_rows)` gallery entries (`INFUR_LOST_WORDS` words each, in gallery order).
    pub fn memory(&self, rows: usize, lost_rows: usize) -> Result<TracksMemory, HipError> {
        let mut out = TracksMemory { gap_of_region: vec![0; rows], summary: [0; 4], lost: vec![0; lost_rows * sys::INFUR_LOST_WORDS as usize] };
        let rc = unsafe {
            sys::infur_tracker_memory(self.raw, if rows > 0 { out.gap_of_region.as_mut_ptr() } else { std::ptr::null_mut() }, rows as u32,
                                      out.summary.as_mut_ptr(), if lost_rows > 0 { out.lost.as_mut_ptr() } else { std::ptr::null_mut() },
                                      lost_rows as u32)
        };
        if rc != sys::INFUR_OK { return Err(HipError::from_ctx(&self.ctx, rc)); }
        out.lost.truncate(out.held().min(lost_rows) * sys::INFUR_LOST_WORDS as usize);
        Ok(out)
    }
}
/// What `HipTracks::memory` reads: see `infur_tracker_memory`.
pub struct TracksMemory { pub gap_of_region: Vec<u32>, pub summary: [u32; 4], pub lost: Vec<u64> }
impl TracksMemory {
    pub fn held(&self) -> usize { self.summary[sys::INFUR_TRACK_MEMORY_HELD as usize] as usize }
    pub fn word(&self, entry: usize, word: u32) -> u64 { self.lost[entry * sys::INFUR_LOST_WORDS as usize + word as usize] }
}
impl Drop for HipTracks {
    fn drop(&mut self) { unsafe { sys::infur_tracker_destroy(self.raw) } }
}
impl Processor for HipTracks {
    type Command = TracksCmd;
    type ControlError = HipError;
    type Input = Regions;
    type Output = Tracks;
    type ProcessResult = Result<(), HipError>;

    fn control(&mut self, cmd: TracksCmd) -> Result<&mut Self, HipError> {
        match cmd {
            TracksCmd::MinOverlap(v) => { self.dirty |= v != self.min_overlap; self.min_overlap = v; }
            TracksCmd::Reset(first_id) => {
                let rc = unsafe { sys::infur_tracker_reset(self.raw, first_id) };
                if rc != sys::INFUR_OK { return Err(HipError::from_ctx(&self.ctx, rc)); }
                self.dirty = true;
            }
        }
        Ok(self)
    }
    fn is_dirty(&self) -> bool { self.dirty }
    fn advance(&mut self, inp: &Regions, out: &mut Tracks) -> Result<(), HipError> {
        self.dirty = false;
        let [w, h] = inp.size;
        if inp.labels.len() != w * h { return Err(HipError::status(sys::INFUR_E_SHAPE)); }  // (Regions made with want_labels)
        let rows = inp.table.len() / sys::INFUR_REGION_WORDS as usize;
        out.rows = if w * h > 0 { (inp.n as usize).min(rows) } else { 0 };
        out.track_of_region.resize(rows, sys::INFUR_TRACK_NONE);
        out.table.resize(rows * sys::INFUR_TRACK_WORDS as usize, 0);
        out.plane.resize(if out.want_plane { h * w } else { 0 }, sys::INFUR_TRACK_NONE);
        let rc = unsafe {
            sys::infur_tracks(self.raw, inp.labels.as_ptr(), inp.table.as_ptr(), rows as u32, inp.n, h as u32, w as u32, self.min_overlap,
                              if rows > 0 { out.track_of_region.as_mut_ptr() } else { std::ptr::null_mut() },
                              if out.want_plane && h * w > 0 { out.plane.as_mut_ptr() } else { std::ptr::null_mut() },
                              if rows > 0 { out.table.as_mut_ptr() } else { std::ptr::null_mut() }, out.summary.as_mut_ptr())
        };
        out.track_of_region.truncate(out.rows);
        out.table.truncate(out.rows * sys::INFUR_TRACK_WORDS as usize);
        if rc == sys::INFUR_OK { Ok(()) } else { Err(HipError::from_ctx(&self.ctx, rc)) }
    }
}

// ---------------------------------------------------------------- Runs (a plane as run-length records)
/// A plane for `HipRuns`: class / confidence bytes or label / track words, with its `size` = [w, h].
pub enum RunsPlaneData { U8(Vec<u8>), U32(Vec<u32>) }
pub struct RunsPlane { pub size: [usize; 2], pub data: RunsPlaneData }
/// What `HipRuns` produces: `runs` holds `min(n, runs_rows)` records of `INFUR_RUN_WORDS` words (START, END, VALUE) in raster
/// order, `row_start` the `h + 1` words of the per-row index, `n` counts every run (above `runs_rows`: truncated).
pub struct Runs { pub runs_rows: usize, pub want_row_start: bool, pub n: u32, pub runs: Vec<u32>, pub row_start: Vec<u32> }
impl Default for Runs {
    fn default() -> Self { Self { runs_rows: 1 << 16, want_row_start: true, n: 0, runs: Vec::new(), row_start: Vec::new() } }
}
impl Runs {
    pub fn rows(&self) -> usize { (self.n as usize).min(self.runs_rows) }
    pub fn word(&self, run: usize, word: u32) -> u32 { self.runs[run * sys::INFUR_RUN_WORDS as usize + word as usize] }
}
pub enum RunsCmd { Skip(u32), NoSkip }
/// The egress stage: runs of equal values within a row, numbered in raster order.  Integer results, identical from run to run.
pub struct HipRuns { ctx: Rc<Ctx>, skip: Option<u32>, dirty: bool }
impl HipRuns {
    pub fn new(ctx: Rc<Ctx>) -> Self { Self { ctx, skip: None, dirty: true } }
}
impl Processor for HipRuns {
    type Command = RunsCmd;
    type ControlError = HipError;
    type Input = RunsPlane;
    type Output = Runs;
    type ProcessResult = Result<(), HipError>;

    fn control(&mut self, cmd: RunsCmd) -> Result<&mut Self, HipError> {
        let skip = match cmd { RunsCmd::Skip(v) => Some(v), RunsCmd::NoSkip => None };
        self.dirty |= skip != self.skip;
        self.skip = skip;
        Ok(self)
    }
    fn is_dirty(&self) -> bool { self.dirty }
    fn advance(&mut self, inp: &RunsPlane, out: &mut Runs) -> Result<(), HipError> {
        self.dirty = false;
        let [w, h] = inp.size;
        let (ptr, len, elem_bytes) = match &inp.data {
            RunsPlaneData::U8(p) => (p.as_ptr() as *const std::ffi::c_void, p.len(), 1u32),
            RunsPlaneData::U32(p) => (p.as_ptr() as *const std::ffi::c_void, p.len(), 4u32),
        };
        if len != w * h { return Err(HipError::status(sys::INFUR_E_SHAPE)); }
        out.runs.resize(out.runs_rows * sys::INFUR_RUN_WORDS as usize, 0);
        out.row_start.resize(if out.want_row_start { h + 1 } else { 0 }, 0);
        let rc = unsafe {
            sys::infur_runs(self.ctx.0, ptr, elem_bytes, h as u32, w as u32, if self.skip.is_some() { sys::INFUR_RUNS_SKIP } else { 0 },
                            self.skip.unwrap_or(0), if out.runs_rows > 0 { out.runs.as_mut_ptr() } else { std::ptr::null_mut() },
                            out.runs_rows as u32, if out.want_row_start { out.row_start.as_mut_ptr() } else { std::ptr::null_mut() },
                            &mut out.n)
        };
        if rc != sys::INFUR_OK { return Err(HipError::from_ctx(&self.ctx, rc)); }
        out.runs.truncate(out.rows() * sys::INFUR_RUN_WORDS as usize);
        Ok(())
    }
}

// ---------------------------------------------------------------- Anchors (a distance transform, one interior point per value)
/// What `HipAnchors` produces: `dist2` holds the `w * h` squared distances to the nearest pixel of another value or to the frame
/// (0: a skipped pixel), `anchors` `rows` rows of `INFUR_ANCHOR_WORDS` words (PIXEL, DIST2), one per value below `rows`;
/// `(INFUR_ANCHOR_NONE, 0)`: no pixel holds the value.
pub struct Anchors { pub rows: usize, pub want_dist2: bool, pub dist2: Vec<u32>, pub anchors: Vec<u32> }
impl Default for Anchors {
    fn default() -> Self { Self { rows: 256, want_dist2: true, dist2: Vec::new(), anchors: Vec::new() } }
}
impl Anchors {
    pub fn word(&self, row: usize, word: u32) -> u32 { self.anchors[row * sys::INFUR_ANCHOR_WORDS as usize + word as usize] }
    /// the anchor of value `row` as (x, y) in a plane of width `w`, `None` where no pixel holds it
    pub fn point(&self, row: usize, w: usize) -> Option<(usize, usize)> {
        let at = self.word(row, sys::INFUR_ANCHOR_PIXEL);
        if at == sys::INFUR_ANCHOR_NONE || w == 0 { None } else { Some((at as usize % w, at as usize / w)) }
    }
}
pub enum AnchorsCmd { Skip(u32), NoSkip }
/// The stage that measures how thick a region is: exact squared distances by value, the frame counting as a border, and per
/// value the most interior pixel (ties to the smallest index).  Integer results, identical from run to run.
pub struct HipAnchors { ctx: Rc<Ctx>, skip: Option<u32>, dirty: bool }
impl HipAnchors {
    pub fn new(ctx: Rc<Ctx>) -> Self { Self { ctx, skip: None, dirty: true } }
}
impl Processor for HipAnchors {
    type Command = AnchorsCmd;
    type ControlError = HipError;
    type Input = RunsPlane;
    type Output = Anchors;
    type ProcessResult = Result<(), HipError>;

    fn control(&mut self, cmd: AnchorsCmd) -> Result<&mut Self, HipError> {
        let skip = match cmd { AnchorsCmd::Skip(v) => Some(v), AnchorsCmd::NoSkip => None };
        self.dirty |= skip != self.skip;
        self.skip = skip;
        Ok(self)
    }
    fn is_dirty(&self) -> bool { self.dirty }
    fn advance(&mut self, inp: &RunsPlane, out: &mut Anchors) -> Result<(), HipError> {
        self.dirty = false;
        let [w, h] = inp.size;
        let (ptr, len, elem_bytes) = match &inp.data {
            RunsPlaneData::U8(p) => (p.as_ptr() as *const std::ffi::c_void, p.len(), 1u32),
            RunsPlaneData::U32(p) => (p.as_ptr() as *const std::ffi::c_void, p.len(), 4u32),
        };
        if len != w * h { return Err(HipError::status(sys::INFUR_E_SHAPE)); }
        out.dist2.resize(if out.want_dist2 { w * h } else { 0 }, 0);
        out.anchors.resize(out.rows * sys::INFUR_ANCHOR_WORDS as usize, 0);
        let rc = unsafe {
            sys::infur_anchors(self.ctx.0, ptr, elem_bytes, h as u32, w as u32, if self.skip.is_some() { sys::INFUR_ANCHORS_SKIP } else { 0 },
                               self.skip.unwrap_or(0), if out.want_dist2 { out.dist2.as_mut_ptr() } else { std::ptr::null_mut() },
                               if out.rows > 0 { out.anchors.as_mut_ptr() } else { std::ptr::null_mut() }, out.rows as u32)
        };
        if rc != sys::INFUR_OK { return Err(HipError::from_ctx(&self.ctx, rc)); }
        Ok(())
    }
}

// ---------------------------------------------------------------- Compare (confusion matrix, best partner per value)
/// What `HipCompare` produces for `rows_a` x `rows_b` values: `matrix` row-major (`matrix[i * rows_b + j]`: the pixels with a == i
/// and b == j), `a` and `b` rows of `INFUR_COMPARE_WORDS` words (PIXELS, PARTNER, INTER, UNION) per value of either plane --
/// `(0, INFUR_COMPARE_NONE, 0, 0)`: no compared pixel holds the value -- and the `INFUR_COMPARE_COUNT_WORDS` counts.
pub struct Compared { pub rows_a: usize, pub rows_b: usize, pub want_matrix: bool, pub matrix: Vec<u32>, pub a: Vec<u32>, pub b: Vec<u32>,
                      pub counts: [u32; sys::INFUR_COMPARE_COUNT_WORDS as usize] }
impl Default for Compared {
    fn default() -> Self {
        Self { rows_a: 21, rows_b: 21, want_matrix: true, matrix: Vec::new(), a: Vec::new(), b: Vec::new(),
               counts: [0; sys::INFUR_COMPARE_COUNT_WORDS as usize] }
    }
}
impl Compared {
    pub fn count(&self, word: u32) -> u32 { self.counts[word as usize] }
    /// the share of compared pixels on which the planes agree
    pub fn pixel_accuracy(&self) -> Option<f64> {
        let n = self.count(sys::INFUR_COMPARE_COMPARED) - self.count(sys::INFUR_COMPARE_OUTSIDE);
        if n == 0 { None } else { Some(self.count(sys::INFUR_COMPARE_EQUAL) as f64 / n as f64) }
    }
    /// row `i` of a's table is matched: 2 INTER > UNION, the rule of panoptic quality
    pub fn matched_a(&self, i: usize) -> bool {
        let r = &self.a[i * sys::INFUR_COMPARE_WORDS as usize..];
        2 * r[sys::INFUR_COMPARE_INTER as usize] as u64 > r[sys::INFUR_COMPARE_UNION as usize] as u64
    }
}
pub enum CompareCmd { Ignore { a: Option<u32>, b: Option<u32> }, PairSlots(u32) }
/// The stage that grades a result: two planes (class, label or track, in any combination) against each other.  Integer results,
/// identical from run to run.
pub struct HipCompare { ctx: Rc<Ctx>, ignore_a: Option<u32>, ignore_b: Option<u32>, pair_slots: u32, dirty: bool }
impl HipCompare {
    pub fn new(ctx: Rc<Ctx>) -> Self { Self { ctx, ignore_a: None, ignore_b: None, pair_slots: 0, dirty: true } }
}
impl Processor for HipCompare {
    type Command = CompareCmd;
    type ControlError = HipError;
    type Input = (RunsPlane, RunsPlane);
    type Output = Compared;
    type ProcessResult = Result<(), HipError>;

    fn control(&mut self, cmd: CompareCmd) -> Result<&mut Self, HipError> {
        match cmd {
            CompareCmd::Ignore { a, b } => {
                self.dirty |= a != self.ignore_a || b != self.ignore_b;
                self.ignore_a = a;
                self.ignore_b = b;
            }
            CompareCmd::PairSlots(n) => {
                self.dirty |= n != self.pair_slots;
                self.pair_slots = n;
            }
        }
        Ok(self)
    }
    fn is_dirty(&self) -> bool { self.dirty }
    fn advance(&mut self, inp: &(RunsPlane, RunsPlane), out: &mut Compared) -> Result<(), HipError> {
        self.dirty = false;
        let [w, h] = inp.0.size;
        if inp.1.size != inp.0.size { return Err(HipError::status(sys::INFUR_E_SHAPE)); }
        let raw = |p: &RunsPlane| match &p.data {
            RunsPlaneData::U8(d) => (d.as_ptr() as *const std::ffi::c_void, d.len(), 1u32),
            RunsPlaneData::U32(d) => (d.as_ptr() as *const std::ffi::c_void, d.len(), 4u32),
        };
        let (pa, la, ea) = raw(&inp.0);
        let (pb, lb, eb) = raw(&inp.1);
        if la != w * h || lb != w * h { return Err(HipError::status(sys::INFUR_E_SHAPE)); }
        let words = sys::INFUR_COMPARE_WORDS as usize;
        out.matrix.resize(if out.want_matrix { out.rows_a * out.rows_b } else { 0 }, 0);
        out.a.resize(out.rows_a * words, 0);
        out.b.resize(out.rows_b * words, 0);
        let flags = (if self.ignore_a.is_some() { sys::INFUR_COMPARE_IGNORE_A } else { 0 })
            | (if self.ignore_b.is_some() { sys::INFUR_COMPARE_IGNORE_B } else { 0 });
        let ptr = |v: &mut Vec<u32>| if v.is_empty() { std::ptr::null_mut() } else { v.as_mut_ptr() };
        let rc = unsafe {
            sys::infur_compare(self.ctx.0, pa, ea, pb, eb, h as u32, w as u32, flags, self.ignore_a.unwrap_or(0), self.ignore_b.unwrap_or(0),
                               ptr(&mut out.matrix), out.rows_a as u32, out.rows_b as u32, ptr(&mut out.a), ptr(&mut out.b),
                               out.counts.as_mut_ptr(), self.pair_slots)
        };
        if rc != sys::INFUR_OK { return Err(HipError::from_ctx(&self.ctx, rc)); }
        Ok(())
    }
}

// ---------------------------------------------------------------- Adjacency (which values touch, along how many pixel edges)
/// What `HipAdjacency` produces for `rows` values: `pairs` holds the `min(PAIRS, pair_rows)` records of `INFUR_ADJ_PAIR_WORDS` words
/// (A < B, BORDER, FIRST) in ascending FIRST, `table` `INFUR_ADJ_ROW_WORDS` words per value (DEGREE, LONGEST, BORDER, PERIMETER;
/// LONGEST == `INFUR_ADJ_NONE`: no neighbour) and the `INFUR_ADJ_COUNT_WORDS` counts.
pub struct Adjacent { pub rows: usize, pub pair_rows: usize, pub pairs: Vec<u32>, pub table: Vec<u32>,
                      pub counts: [u32; sys::INFUR_ADJ_COUNT_WORDS as usize] }
impl Default for Adjacent {
    fn default() -> Self {
        Self { rows: 21, pair_rows: 4096, pairs: Vec::new(), table: Vec::new(), counts: [0; sys::INFUR_ADJ_COUNT_WORDS as usize] }
    }
}
impl Adjacent {
    pub fn count(&self, word: u32) -> u32 { self.counts[word as usize] }
    /// the neighbours of `value` with their borders, longest first and then by value: the head is the row table's LONGEST
    pub fn neighbours(&self, value: u32) -> Vec<(u32, u32)> {
        let mut v: Vec<(u32, u32)> = self.pairs.chunks_exact(sys::INFUR_ADJ_PAIR_WORDS as usize).filter_map(|p| {
            if p[0] == value { Some((p[1], p[2])) } else if p[1] == value { Some((p[0], p[2])) } else { None }
        }).collect();
        v.sort_by(|x, y| y.1.cmp(&x.1).then(x.0.cmp(&y.0)));
        v
    }
}
pub enum AdjacencyCmd { Skip(u32), NoSkip, PairSlots(u32) }
/// The region adjacency graph of a class, label or track plane.  Integer results, identical from run to run.
pub struct HipAdjacency { ctx: Rc<Ctx>, skip: Option<u32>, pair_slots: u32, dirty: bool }
impl HipAdjacency {
    pub fn new(ctx: Rc<Ctx>) -> Self { Self { ctx, skip: None, pair_slots: 0, dirty: true } }
}
impl Processor for HipAdjacency {
    type Command = AdjacencyCmd;
    type ControlError = HipError;
    type Input = RunsPlane;
    type Output = Adjacent;
    type ProcessResult = Result<(), HipError>;

    fn control(&mut self, cmd: AdjacencyCmd) -> Result<&mut Self, HipError> {
        let (skip, slots) = match cmd {
            AdjacencyCmd::Skip(v) => (Some(v), self.pair_slots),
            AdjacencyCmd::NoSkip => (None, self.pair_slots),
            AdjacencyCmd::PairSlots(n) => (self.skip, n),
        };
        self.dirty |= skip != self.skip || slots != self.pair_slots;
        self.skip = skip;
        self.pair_slots = slots;
        Ok(self)
    }
    fn is_dirty(&self) -> bool { self.dirty }
    fn advance(&mut self, inp: &RunsPlane, out: &mut Adjacent) -> Result<(), HipError> {
        self.dirty = false;
        let [w, h] = inp.size;
        let (ptr, len, elem) = match &inp.data {
            RunsPlaneData::U8(d) => (d.as_ptr() as *const std::ffi::c_void, d.len(), 1u32),
            RunsPlaneData::U32(d) => (d.as_ptr() as *const std::ffi::c_void, d.len(), 4u32),
        };
        if len != w * h { return Err(HipError::status(sys::INFUR_E_SHAPE)); }
        out.pairs.clear();
        out.pairs.resize(out.pair_rows.max(1) * sys::INFUR_ADJ_PAIR_WORDS as usize, 0);  // (a pointer also for zero records)
        out.table.resize(out.rows * sys::INFUR_ADJ_ROW_WORDS as usize, 0);
        let rc = unsafe {
            sys::infur_adjacency(self.ctx.0, ptr, elem, h as u32, w as u32, if self.skip.is_some() { sys::INFUR_ADJ_SKIP } else { 0 },
                                 self.skip.unwrap_or(0), out.rows as u32, out.pairs.as_mut_ptr(), out.pair_rows as u32,
                                 if out.table.is_empty() { std::ptr::null_mut() } else { out.table.as_mut_ptr() }, out.counts.as_mut_ptr(),
                                 self.pair_slots)
        };
        if rc != sys::INFUR_OK { out.pairs.clear(); return Err(HipError::from_ctx(&self.ctx, rc)); }
        out.pairs.truncate(out.counts[sys::INFUR_ADJ_WRITTEN as usize] as usize * sys::INFUR_ADJ_PAIR_WORDS as usize);
        Ok(())
    }
}

// ---------------------------------------------------------------- Sieve (speckle regions merged into their neighbours)
/// What `HipSieve` consumes: the class plane and what `HipRegions` made of it with `min_pixels` 0, no background skip and
/// `want_labels`.
pub struct SieveInput { pub klass: Vec<u8>, pub regions: Regions }
/// What `HipSieve` produces: `klass` the cleaned `h * w` class plane, `rows` `INFUR_SIEVE_ROW_WORDS` words per region (CLASS, INTO,
/// ROUND, BORDER; ROUND == `INFUR_SIEVE_NONE`: stranded) and the `INFUR_SIEVE_COUNT_WORDS` counts.
#[derive(Default)]
pub struct Sieved { pub size: [usize; 2], pub klass: Vec<u8>, pub rows: Vec<u32>, pub counts: [u32; sys::INFUR_SIEVE_COUNT_WORDS as usize] }
impl Sieved {
    pub fn count(&self, word: u32) -> u32 { self.counts[word as usize] }
    pub fn word(&self, region: usize, word: u32) -> u32 { self.rows[region * sys::INFUR_SIEVE_ROW_WORDS as usize + word as usize] }
}
pub enum SieveCmd { MinPixels(u32), MaxRounds(u32), PairSlots(u32) }
/// The stage that removes speckle: every region of fewer than `min_pixels` pixels takes the class of the neighbour it shares the
/// longest border with, round by round.  Integer results, identical from run to run.
pub struct HipSieve { ctx: Rc<Ctx>, min_pixels: u32, max_rounds: u32, pair_slots: u32, dirty: bool }
impl HipSieve {
    pub fn new(ctx: Rc<Ctx>) -> Self { Self { ctx, min_pixels: 0, max_rounds: 0, pair_slots: 0, dirty: true } }
}
impl Processor for HipSieve {
    type Command = SieveCmd;
    type ControlError = HipError;
    type Input = SieveInput;
    type Output = Sieved;
    type ProcessResult = Result<(), HipError>;

    fn control(&mut self, cmd: SieveCmd) -> Result<&mut Self, HipError> {
        let (minpx, rounds, slots) = match cmd {
            SieveCmd::MinPixels(n) => (n, self.max_rounds, self.pair_slots),
            SieveCmd::MaxRounds(n) => {
                if n > 64 { return Err(HipError::status(sys::INFUR_E_INVALID_ARG)); }  // state untouched
                (self.min_pixels, n, self.pair_slots)
            }
            SieveCmd::PairSlots(n) => (self.min_pixels, self.max_rounds, n),
        };
        self.dirty |= (minpx, rounds, slots) != (self.min_pixels, self.max_rounds, self.pair_slots);
        self.min_pixels = minpx;
        self.max_rounds = rounds;
        self.pair_slots = slots;
        Ok(self)
    }
    fn is_dirty(&self) -> bool { self.dirty }
    fn advance(&mut self, inp: &SieveInput, out: &mut Sieved) -> Result<(), HipError> {
        self.dirty = false;
        let [w, h] = inp.regions.size;
        if inp.klass.len() != w * h || inp.regions.labels.len() != w * h { return Err(HipError::status(sys::INFUR_E_SHAPE)); }
        out.size = inp.regions.size;
        out.klass.resize(w * h, 0);
        out.rows.resize(inp.regions.rows() * sys::INFUR_SIEVE_ROW_WORDS as usize, 0);
        let rc = unsafe {
            sys::infur_sieve(self.ctx.0, inp.klass.as_ptr(), inp.regions.labels.as_ptr(), inp.regions.table.as_ptr(), inp.regions.table_rows as u32,
                             inp.regions.n, h as u32, w as u32, self.min_pixels, self.max_rounds, self.pair_slots,
                             if out.klass.is_empty() { std::ptr::null_mut() } else { out.klass.as_mut_ptr() },
                             if out.rows.is_empty() { std::ptr::null_mut() } else { out.rows.as_mut_ptr() }, out.counts.as_mut_ptr())
        };
        if rc != sys::INFUR_OK { return Err(HipError::from_ctx(&self.ctx, rc)); }
        Ok(())
    }
}

// ---------------------------------------------------------------- Outlines (region boundaries as polygon loops)
/// What `HipOutlines` produces: `loops` holds `min(n_loops, loops_rows)` records of `INFUR_LOOP_WORDS` words (OFFSET, COUNT, VALUE,
/// START), `vertices` the first `min(n_vertices, vertex_rows)` vertex ids `Y*(w+1) + X`, loops back to back; the three counts are
/// complete whatever the rows are (`n_loops == 0 && n_edges > 0`: the edges exceeded `max_edges`).
pub struct Outlines { pub loops_rows: usize, pub vertex_rows: usize, pub n_loops: u32, pub n_vertices: u32, pub n_edges: u32,
                      pub loops: Vec<u32>, pub vertices: Vec<u32> }
impl Default for Outlines {
    fn default() -> Self {
        Self { loops_rows: 1 << 16, vertex_rows: 1 << 20, n_loops: 0, n_vertices: 0, n_edges: 0, loops: Vec::new(), vertices: Vec::new() }
    }
}
impl Outlines {
    pub fn rows(&self) -> usize { (self.n_loops as usize).min(self.loops_rows) }
    pub fn word(&self, l: usize, word: u32) -> u32 { self.loops[l * sys::INFUR_LOOP_WORDS as usize + word as usize] }
    /// the boundary of a hole (counter-clockwise on a y-down screen)
    pub fn is_hole(&self, l: usize) -> bool { self.word(l, sys::INFUR_LOOP_START) & 3 == 2 }
}
pub enum OutlinesCmd { Skip(u32), NoSkip, Connectivity(u32), MaxEdges(u32) }
/// The polygon stage: the boundaries of the value-regions of a plane as closed loops.  Integer results, identical from run to run.
pub struct HipOutlines { ctx: Rc<Ctx>, skip: Option<u32>, conn8: bool, max_edges: u32, dirty: bool }
impl HipOutlines {
    pub fn new(ctx: Rc<Ctx>) -> Self { Self { ctx, skip: None, conn8: false, max_edges: 0, dirty: true } }
}
impl Processor for HipOutlines {
    type Command = OutlinesCmd;
    type ControlError = HipError;
    type Input = RunsPlane;
    type Output = Outlines;
    type ProcessResult = Result<(), HipError>;

    fn control(&mut self, cmd: OutlinesCmd) -> Result<&mut Self, HipError> {
        let (skip, conn8, max_edges) = match cmd {
            OutlinesCmd::Skip(v) => (Some(v), self.conn8, self.max_edges),
            OutlinesCmd::NoSkip => (None, self.conn8, self.max_edges),
            OutlinesCmd::Connectivity(4) => (self.skip, false, self.max_edges),
            OutlinesCmd::Connectivity(8) => (self.skip, true, self.max_edges),
            OutlinesCmd::Connectivity(_) => return Err(HipError::status(sys::INFUR_E_INVALID_ARG)),
            OutlinesCmd::MaxEdges(n) => (self.skip, self.conn8, n),
        };
        self.dirty |= (skip, conn8, max_edges) != (self.skip, self.conn8, self.max_edges);
        self.skip = skip;
        self.conn8 = conn8;
        self.max_edges = max_edges;
        Ok(self)
    }
    fn is_dirty(&self) -> bool { self.dirty }
    fn advance(&mut self, inp: &RunsPlane, out: &mut Outlines) -> Result<(), HipError> {
        self.dirty = false;
        let [w, h] = inp.size;
        let (ptr, len, elem_bytes) = match &inp.data {
            RunsPlaneData::U8(p) => (p.as_ptr() as *const std::ffi::c_void, p.len(), 1u32),
            RunsPlaneData::U32(p) => (p.as_ptr() as *const std::ffi::c_void, p.len(), 4u32),
        };
        if len != w * h { return Err(HipError::status(sys::INFUR_E_SHAPE)); }
        out.loops.resize(out.loops_rows * sys::INFUR_LOOP_WORDS as usize, 0);
        out.vertices.resize(out.vertex_rows, 0);
        let mut counts = [0u32; 3];
        let flags = if self.skip.is_some() { sys::INFUR_OUTLINES_SKIP } else { 0 } | if self.conn8 { sys::INFUR_OUTLINES_CONN8 } else { 0 };
        let rc = unsafe {
            sys::infur_outlines(self.ctx.0, ptr, elem_bytes, h as u32, w as u32, flags, self.skip.unwrap_or(0), self.max_edges,
                                if out.loops_rows > 0 { out.loops.as_mut_ptr() } else { std::ptr::null_mut() }, out.loops_rows as u32,
                                if out.vertex_rows > 0 { out.vertices.as_mut_ptr() } else { std::ptr::null_mut() }, out.vertex_rows as u32,
                                counts.as_mut_ptr())
        };
        if rc != sys::INFUR_OK { return Err(HipError::from_ctx(&self.ctx, rc)); }
        out.n_loops = counts[0];
        out.n_vertices = counts[1];
        out.n_edges = counts[2];
        out.loops.truncate(out.rows() * sys::INFUR_LOOP_WORDS as usize);
        out.vertices.truncate((out.n_vertices as usize).min(out.vertex_rows));
        Ok(())
    }
}

// ---------------------------------------------------------------- Simplify (Outlines' loops within a tolerance)
/// What `HipSimplify` produces, in `Outlines`' layout: `loops` holds `min(n_loops, loops_rows)` records (OFFSET', COUNT', VALUE,
/// START), `vertices` the first `min(n_vertices, vertex_rows)` kept vertex ids; `n_degenerate` counts the loops with COUNT' < 3
/// (skip them); `status`: `INFUR_SIMPLIFY_TRUNCATED` (the input was cut off: nothing was produced), `INFUR_SIMPLIFY_MALFORMED`.
pub struct Simplified { pub loops_rows: usize, pub vertex_rows: usize, pub n_loops: u32, pub n_vertices: u32, pub n_degenerate: u32,
                        pub status: u32, pub loops: Vec<u32>, pub vertices: Vec<u32> }
impl Default for Simplified {
    fn default() -> Self {
        Self { loops_rows: 1 << 16, vertex_rows: 1 << 20, n_loops: 0, n_vertices: 0, n_degenerate: 0, status: 0, loops: Vec::new(),
               vertices: Vec::new() }
    }
}
impl Simplified {
    pub fn rows(&self) -> usize {
        if self.status & sys::INFUR_SIMPLIFY_TRUNCATED != 0 { 0 } else { (self.n_loops as usize).min(self.loops_rows) }
    }
    pub fn word(&self, l: usize, word: u32) -> u32 { self.loops[l * sys::INFUR_LOOP_WORDS as usize + word as usize] }
    /// a thin region that collapsed to its two anchors: no polygon
    pub fn is_degenerate(&self, l: usize) -> bool { self.word(l, sys::INFUR_LOOP_COUNT) < 3 }
}
/// `Outlines` as `HipOutlines` left them, and the plane's `[width, height]`
pub struct SimplifyInput { pub outlines: Outlines, pub size: [usize; 2] }
pub enum SimplifyCmd { Tol16(u32) }
/// Douglas-Peucker on every loop within `tol16` sixteenths of a pixel.  Integer results, identical from run to run; topology is
/// not preserved.
pub struct HipSimplify { ctx: Rc<Ctx>, tol16: u32, dirty: bool }
impl HipSimplify {
    pub fn new(ctx: Rc<Ctx>) -> Self { Self { ctx, tol16: 16, dirty: true } }
}
impl Processor for HipSimplify {
    type Command = SimplifyCmd;
    type ControlError = HipError;
    type Input = SimplifyInput;
    type Output = Simplified;
    type ProcessResult = Result<(), HipError>;

    fn control(&mut self, cmd: SimplifyCmd) -> Result<&mut Self, HipError> {
        let SimplifyCmd::Tol16(t) = cmd;
        if t > 65535 { return Err(HipError::status(sys::INFUR_E_INVALID_ARG)); }
        self.dirty |= t != self.tol16;
        self.tol16 = t;
        Ok(self)
    }
    fn is_dirty(&self) -> bool { self.dirty }
    fn advance(&mut self, inp: &SimplifyInput, out: &mut Simplified) -> Result<(), HipError> {
        self.dirty = false;
        let [w, h] = inp.size;
        let o = &inp.outlines;
        let rows_in = o.loops.len() / sys::INFUR_LOOP_WORDS as usize;
        let lrows = out.loops_rows.min(rows_in);
        let vrows = out.vertex_rows.min(o.vertices.len());
        out.loops.resize(lrows * sys::INFUR_LOOP_WORDS as usize, 0);
        out.vertices.resize(vrows, 0);
        let counts_in = [o.n_loops, o.n_vertices];
        let mut counts = [0u32; 4];
        let rc = unsafe {
            sys::infur_simplify(self.ctx.0, if rows_in > 0 { o.loops.as_ptr() } else { std::ptr::null() }, rows_in as u32,
                                if !o.vertices.is_empty() { o.vertices.as_ptr() } else { std::ptr::null() }, o.vertices.len() as u32,
                                counts_in.as_ptr(), h as u32, w as u32, self.tol16,
                                if lrows > 0 { out.loops.as_mut_ptr() } else { std::ptr::null_mut() }, lrows as u32,
                                if vrows > 0 { out.vertices.as_mut_ptr() } else { std::ptr::null_mut() }, vrows as u32, counts.as_mut_ptr())
        };
        if rc != sys::INFUR_OK { return Err(HipError::from_ctx(&self.ctx, rc)); }
        out.n_loops = counts[0];
        out.n_vertices = counts[1];
        out.n_degenerate = counts[2];
        out.status = counts[3];
        let nl = if out.status & sys::INFUR_SIMPLIFY_TRUNCATED != 0 { 0 } else { (out.n_loops as usize).min(lrows) };
        out.loops.truncate(nl * sys::INFUR_LOOP_WORDS as usize);
        out.vertices.truncate((out.n_vertices as usize).min(vrows));
        Ok(())
    }
}

// ---------------------------------------------------------------- Shapes (hull, moments and rectangle per loop)
/// What `HipShapes` produces: the hulls in `Outlines`' layout (`loops`, `vertices`), `shapes` with `INFUR_SHAPE_WORDS` signed words
/// per loop (AREA2 .. RECT_L) and `values` with as many per value (words 8 .. 10: OUTER, HOLES, LOOP), every one of `value_rows`
/// written; `status`: `INFUR_SHAPES_TRUNCATED` (the input was cut off), `INFUR_SHAPES_MALFORMED`; `largest`: the largest COUNT'.
pub struct Shaped { pub loops_rows: usize, pub vertex_rows: usize, pub shape_rows: usize, pub value_rows: usize, pub n_loops: u32,
                    pub n_vertices: u32, pub status: u32, pub largest: u32, pub loops: Vec<u32>, pub vertices: Vec<u32>, pub shapes: Vec<i64>,
                    pub values: Vec<i64> }
impl Default for Shaped {
    fn default() -> Self {
        Self { loops_rows: 1 << 16, vertex_rows: 1 << 20, shape_rows: 1 << 16, value_rows: 0, n_loops: 0, n_vertices: 0, status: 0, largest: 0,
               loops: Vec::new(), vertices: Vec::new(), shapes: Vec::new(), values: Vec::new() }
    }
}
impl Shaped {
    pub fn shape_word(&self, l: usize, word: u32) -> i64 { self.shapes[l * sys::INFUR_SHAPE_WORDS as usize + word as usize] }
    pub fn value_word(&self, v: usize, word: u32) -> i64 { self.values[v * sys::INFUR_SHAPE_WORDS as usize + word as usize] }
}
/// The descriptor stage behind `HipOutlines`; its input is `HipSimplify`'s.  No command.  Integer results, identical from run to run.
pub struct HipShapes { ctx: Rc<Ctx>, dirty: bool }
impl HipShapes {
    pub fn new(ctx: Rc<Ctx>) -> Self { Self { ctx, dirty: true } }
}
impl Processor for HipShapes {
    type Command = ();
    type ControlError = HipError;
    type Input = SimplifyInput;
    type Output = Shaped;
    type ProcessResult = Result<(), HipError>;

    fn control(&mut self, _cmd: ()) -> Result<&mut Self, HipError> { Ok(self) }
    fn is_dirty(&self) -> bool { self.dirty }
    fn advance(&mut self, inp: &SimplifyInput, out: &mut Shaped) -> Result<(), HipError> {
        self.dirty = false;
        let [w, h] = inp.size;
        let o = &inp.outlines;
        let words = sys::INFUR_SHAPE_WORDS as usize;
        let rows_in = o.loops.len() / sys::INFUR_LOOP_WORDS as usize;
        let lrows = out.loops_rows.min(rows_in);
        let vrows = out.vertex_rows.min(o.vertices.len());
        let srows = out.shape_rows.min(rows_in);
        out.loops.resize(lrows * sys::INFUR_LOOP_WORDS as usize, 0);
        out.vertices.resize(vrows, 0);
        out.shapes.resize(srows * words, 0);
        out.values.resize(out.value_rows * words, 0);
        let counts_in = [o.n_loops, o.n_vertices];
        let mut counts = [0u32; 4];
        let rc = unsafe {
            sys::infur_shapes(self.ctx.0, if rows_in > 0 { o.loops.as_ptr() } else { std::ptr::null() }, rows_in as u32,
                              if !o.vertices.is_empty() { o.vertices.as_ptr() } else { std::ptr::null() }, o.vertices.len() as u32,
                              counts_in.as_ptr(), h as u32, w as u32,
                              if lrows > 0 { out.loops.as_mut_ptr() } else { std::ptr::null_mut() }, lrows as u32,
                              if vrows > 0 { out.vertices.as_mut_ptr() } else { std::ptr::null_mut() }, vrows as u32,
                              if srows > 0 { out.shapes.as_mut_ptr() as *mut u64 } else { std::ptr::null_mut() }, srows as u32,
                              if out.value_rows > 0 { out.values.as_mut_ptr() as *mut u64 } else { std::ptr::null_mut() }, out.value_rows as u32,
                              counts.as_mut_ptr())
        };
        if rc != sys::INFUR_OK { return Err(HipError::from_ctx(&self.ctx, rc)); }
        out.n_loops = counts[sys::INFUR_SHAPES_LOOPS as usize];
        out.n_vertices = counts[sys::INFUR_SHAPES_VERTICES as usize];
        out.status = counts[sys::INFUR_SHAPES_STATUS as usize];
        out.largest = counts[sys::INFUR_SHAPES_LARGEST as usize];
        let cut = out.status & sys::INFUR_SHAPES_TRUNCATED != 0;
        out.loops.truncate(if cut { 0 } else { (out.n_loops as usize).min(lrows) } * sys::INFUR_LOOP_WORDS as usize);
        out.vertices.truncate((out.n_vertices as usize).min(vrows));
        out.shapes.truncate(if cut { 0 } else { (out.n_loops as usize).min(srows) } * words);
        Ok(())
    }
}

// ---------------------------------------------------------------- Raster (loops and runs back into a plane)
/// What `HipRaster` reads: the loops of a polygon stage (`Loops`, `HipSimplify`'s input) or the records of `HipRuns` with the plane's
/// `[w, h]`.
pub enum RasterInput { Loops(SimplifyInput), Runs { runs: Runs, size: [usize; 2] } }
/// What `HipRaster` produces: `plane` holds `h * w` elements of `elem_bytes` bytes each (empty when the input was truncated),
/// `painted` and `conflict` count the pixels exactly one loop claims and the pixels that were refused (overlaps, a hole alone,
/// crossed arcs, a value a byte plane cannot hold); `status`: `INFUR_RASTER_TRUNCATED`, `_MALFORMED`, `_OUTSIDE`.
#[derive(Default)]
pub struct Rastered { pub n: u32, pub painted: u32, pub conflict: u32, pub status: u32, pub plane: Vec<u8> }
pub enum RasterCmd { Fill { elem_bytes: u32, fill_value: u32 } }
/// The stage that goes the other way: polygon loops or run-length records filled into a plane.  Winding 1 paints the loop's value,
/// everything else reads `fill_value`.  Integer results, identical from run to run.
pub struct HipRaster { ctx: Rc<Ctx>, elem_bytes: u32, fill_value: u32, dirty: bool }
impl HipRaster {
    pub fn new(ctx: Rc<Ctx>) -> Self { Self { ctx, elem_bytes: 1, fill_value: 0, dirty: true } }
}
impl Processor for HipRaster {
    type Command = RasterCmd;
    type ControlError = HipError;
    type Input = RasterInput;
    type Output = Rastered;
    type ProcessResult = Result<(), HipError>;

    fn control(&mut self, cmd: RasterCmd) -> Result<&mut Self, HipError> {
        let RasterCmd::Fill { elem_bytes, fill_value } = cmd;
        if (elem_bytes != 1 && elem_bytes != 4) || (elem_bytes == 1 && fill_value > 255) {
            return Err(HipError::status(sys::INFUR_E_INVALID_ARG));
        }
        self.dirty = self.dirty || elem_bytes != self.elem_bytes || fill_value != self.fill_value;
        self.elem_bytes = elem_bytes;
        self.fill_value = fill_value;
        Ok(self)
    }
    fn is_dirty(&self) -> bool { self.dirty }
    fn advance(&mut self, inp: &RasterInput, out: &mut Rastered) -> Result<(), HipError> {
        self.dirty = false;
        let [w, h] = match inp { RasterInput::Loops(l) => l.size, RasterInput::Runs { size, .. } => *size };
        out.plane.resize(w * h * self.elem_bytes as usize, 0);
        let mut counts = [0u32; 4];
        let plane = if out.plane.is_empty() { std::ptr::null_mut() } else { out.plane.as_mut_ptr() as *mut std::ffi::c_void };
        let rc = match inp {
            RasterInput::Loops(l) => {
                let o = &l.outlines;
                let rows_in = o.loops.len() / sys::INFUR_LOOP_WORDS as usize;
                let counts_in = [o.n_loops, o.n_vertices];
                unsafe {
                    sys::infur_raster(self.ctx.0, if rows_in > 0 { o.loops.as_ptr() } else { std::ptr::null() }, rows_in as u32,
                                      if !o.vertices.is_empty() { o.vertices.as_ptr() } else { std::ptr::null() }, o.vertices.len() as u32,
                                      counts_in.as_ptr(), h as u32, w as u32, self.elem_bytes, self.fill_value, plane, counts.as_mut_ptr())
                }
            }
            RasterInput::Runs { runs, .. } => {
                let rows_in = runs.runs.len() / sys::INFUR_RUN_WORDS as usize;
                unsafe {
                    sys::infur_raster_runs(self.ctx.0, if rows_in > 0 { runs.runs.as_ptr() } else { std::ptr::null() }, rows_in as u32, runs.n,
                                           h as u32, w as u32, self.elem_bytes, self.fill_value, plane, counts.as_mut_ptr())
                }
            }
        };
        if rc != sys::INFUR_OK { return Err(HipError::from_ctx(&self.ctx, rc)); }
        out.n = counts[sys::INFUR_RASTER_LOOPS as usize];
        out.painted = counts[sys::INFUR_RASTER_PAINTED as usize];
        out.conflict = counts[sys::INFUR_RASTER_CONFLICT as usize];
        out.status = counts[sys::INFUR_RASTER_STATUS as usize];
        if out.status & sys::INFUR_RASTER_TRUNCATED != 0 { out.plane.clear(); }
        Ok(())
    }
}

// ---------------------------------------------------------------- Coverage (shared borders simplified once)
/// What `HipCoverage` produces, in `Outlines`' layout: `loops` holds `min(n_loops, loops_rows)` records (OFFSET', COUNT', VALUE,
/// START), `vertices` the first `min(n_vertices, vertex_rows)` kept vertex ids; `n_degenerate` counts the loops with COUNT' < 3
/// (skip them); `status`: `INFUR_COVERAGE_TRUNCATED` and `INFUR_COVERAGE_OVERFLOW` (nothing was produced),
/// `INFUR_COVERAGE_MALFORMED`; `n_aug`: the vertices once the junctions were inserted; `n_arcs`: a ring counts as one.
pub struct Covered {
    pub loops_rows: usize, pub vertex_rows: usize,
    pub loops: Vec<u32>, pub vertices: Vec<u32>,
    pub n_loops: u32, pub n_vertices: u32, pub n_degenerate: u32, pub status: u32, pub n_aug: u32, pub n_arcs: u32,
}
impl Covered {
    pub fn new(loops_rows: usize, vertex_rows: usize) -> Self {
        Self { loops_rows, vertex_rows, loops: Vec::new(), vertices: Vec::new(), n_loops: 0, n_vertices: 0, n_degenerate: 0, status: 0, n_aug: 0, n_arcs: 0 }
    }
    pub fn rows(&self) -> usize {
        if self.status & (sys::INFUR_COVERAGE_TRUNCATED | sys::INFUR_COVERAGE_OVERFLOW) != 0 { 0 } else { (self.n_loops as usize).min(self.loops_rows) }
    }
    pub fn word(&self, l: usize, word: u32) -> u32 { self.loops[l * sys::INFUR_LOOP_WORDS as usize + word as usize] }
    pub fn is_degenerate(&self, l: usize) -> bool { self.word(l, sys::INFUR_LOOP_COUNT) < 3 }
}
/// the plane `HipOutlines` was given, and the `Outlines` it left
pub struct CoverageInput { pub plane: RunsPlane, pub outlines: Outlines }
pub enum CoverageCmd { Tol16(u32), Skip(u32), NoSkip, AugRows(u32) }
/// `HipSimplify`'s sibling: the loops are cut at the plane's junctions and every arc is simplified once within `tol16` sixteenths
/// of a pixel, so that neighbouring polygons still share their borders.  Integer results, identical from run to run.
pub struct HipCoverage { ctx: Rc<Ctx>, tol16: u32, skip: Option<u32>, aug_rows: u32, dirty: bool }
impl HipCoverage {
    pub fn new(ctx: Rc<Ctx>) -> Self { Self { ctx, tol16: 16, skip: None, aug_rows: 0, dirty: true } }
}
impl Processor for HipCoverage {
    type Command = CoverageCmd;
    type ControlError = HipError;
    type Input = CoverageInput;
    type Output = Covered;
    type ProcessResult = Result<(), HipError>;

    fn control(&mut self, cmd: CoverageCmd) -> Result<&mut Self, HipError> {
        let (tol16, skip, aug_rows) = match cmd {
            CoverageCmd::Tol16(t) if t > 65535 => return Err(HipError::status(sys::INFUR_E_INVALID_ARG)),
            CoverageCmd::Tol16(t) => (t, self.skip, self.aug_rows),
            CoverageCmd::Skip(v) => (self.tol16, Some(v), self.aug_rows),
            CoverageCmd::NoSkip => (self.tol16, None, self.aug_rows),
            CoverageCmd::AugRows(n) => (self.tol16, self.skip, n),
        };
        self.dirty |= (tol16, skip, aug_rows) != (self.tol16, self.skip, self.aug_rows);
        self.tol16 = tol16;
        self.skip = skip;
        self.aug_rows = aug_rows;
        Ok(self)
    }
    fn is_dirty(&self) -> bool { self.dirty }
    fn advance(&mut self, inp: &CoverageInput, out: &mut Covered) -> Result<(), HipError> {
        self.dirty = false;
        let [w, h] = inp.plane.size;
        let (ptr, len, elem_bytes) = match &inp.plane.data {
            RunsPlaneData::U8(p) => (p.as_ptr() as *const std::ffi::c_void, p.len(), 1u32),
            RunsPlaneData::U32(p) => (p.as_ptr() as *const std::ffi::c_void, p.len(), 4u32),
        };
        if len != w * h { return Err(HipError::status(sys::INFUR_E_SHAPE)); }
        let o = &inp.outlines;
        let rows_in = o.loops.len() / sys::INFUR_LOOP_WORDS as usize;
        let lrows = out.loops_rows.min(rows_in);
        let vrows = out.vertex_rows.min(o.vertices.len() + (w + 1) * (h + 1));  // junctions are inserted
        out.loops.resize(lrows * sys::INFUR_LOOP_WORDS as usize, 0);
        out.vertices.resize(vrows, 0);
        let counts_in = [o.n_loops, o.n_vertices];
        let mut counts = [0u32; 6];
        let rc = unsafe {
            sys::infur_coverage(self.ctx.0, ptr, elem_bytes, h as u32, w as u32, if self.skip.is_some() { sys::INFUR_COVERAGE_SKIP } else { 0 },
                                self.skip.unwrap_or(0), if rows_in > 0 { o.loops.as_ptr() } else { std::ptr::null() }, rows_in as u32,
                                if !o.vertices.is_empty() { o.vertices.as_ptr() } else { std::ptr::null() }, o.vertices.len() as u32,
                                counts_in.as_ptr(), self.tol16, self.aug_rows,
                                if lrows > 0 { out.loops.as_mut_ptr() } else { std::ptr::null_mut() }, lrows as u32,
                                if vrows > 0 { out.vertices.as_mut_ptr() } else { std::ptr::null_mut() }, vrows as u32, counts.as_mut_ptr())
        };
        if rc != sys::INFUR_OK { return Err(HipError::from_ctx(&self.ctx, rc)); }
        out.n_loops = counts[0];
        out.n_vertices = counts[1];
        out.n_degenerate = counts[2];
        out.status = counts[3];
        out.n_aug = counts[4];
        out.n_arcs = counts[5];
        let nothing = out.status & (sys::INFUR_COVERAGE_TRUNCATED | sys::INFUR_COVERAGE_OVERFLOW) != 0;
        let nl = if nothing { 0 } else { (out.n_loops as usize).min(lrows) };
        out.loops.truncate(nl * sys::INFUR_LOOP_WORDS as usize);
        out.vertices.truncate((out.n_vertices as usize).min(vrows));
        Ok(())
    }
}

// ---------------------------------------------------------------- streaming ring with zero-copy slots (main.rs:27-99,105; ABI 5)
/// The bounded queue of frames in flight (`sync_channel(2)`, main.rs:105) over `infur_stream_*`.  `next_slot` / `commit` let the
/// decoder fill the ring's own pinned buffer in place -- what `ff-video/src/decoder.rs:156-165` does with its reused `BgrImage` --
/// and `view` / `release` hand the finished mask out of the pinned output slot: no pageable <-> pinned copy on either side.
/// UNTESTED like the rest of the crate (no Rust toolchain in the build image).
pub struct HipStream { raw: *mut sys::infur_stream, ctx: Rc<Ctx>, depth: u32, mode: u32 }
/// A finished frame in place in the ring's pinned output slot; the slot returns to the ring when the view is dropped.
pub struct MaskView<'a> { stream: &'a mut HipStream, pub frame_id: u64, pub size: [usize; 2], pub rgba: &'a [u8], pub scaled_bgr: Option<&'a [u8]> }
impl<'a> Drop for MaskView<'a> {
    fn drop(&mut self) { unsafe { sys::infur_stream_release(self.stream.raw); } }
}
impl HipStream {
    pub fn new(ctx: Rc<Ctx>, depth: u32) -> Result<Self, HipError> {
        let mut raw = std::ptr::null_mut();
        let rc = unsafe { sys::infur_stream_create(ctx.0, depth, &mut raw) };
        if rc != sys::INFUR_OK { return Err(HipError::from_ctx(&ctx, rc)); }
        Ok(Self { raw, ctx, depth, mode: sys::INFUR_SCALE_NEAREST })
    }
    pub fn pending(&self) -> u32 { unsafe { sys::infur_stream_pending(self.raw) } }
    pub fn depth(&self) -> u32 { self.depth }
    /// the next slot's pinned input buffer, `w * h * 3` bytes of packed bgr24 for the decoder to `read_exact` into
    pub fn next_slot(&mut self, w: u32, h: u32, factor: f32) -> Result<&mut [u8], HipError> {
        let mut p: *mut u8 = std::ptr::null_mut();
        let rc = unsafe { sys::infur_stream_acquire(self.raw, w, h, factor, &mut p) };
        if rc != sys::INFUR_OK { return Err(HipError::from_ctx(&self.ctx, rc)); }
        Ok(unsafe { std::slice::from_raw_parts_mut(p, (w as usize) * (h as usize) * 3) })
    }
    pub fn commit(&mut self, w: u32, h: u32, factor: f32, frame_id: u64) -> Result<(), HipError> {
        let rc = unsafe { sys::infur_stream_commit(self.raw, w, h, factor, self.mode, frame_id) };
        if rc != sys::INFUR_OK { return Err(HipError::from_ctx(&self.ctx, rc)); }
        Ok(())
    }
    /// the decoder found no frame for the slot `next_slot` lent out (end of input, read error): give it back uncommitted, so that
    /// copying `submit`s work again on this stream
    pub fn abandon(&mut self) { unsafe { sys::infur_stream_abandon(self.raw); } }
    /// waits for the oldest pending frame
    pub fn view(&mut self) -> Result<MaskView<'_>, HipError> {
        let (mut rgba, mut sc): (*const u8, *const u8) = (std::ptr::null(), std::ptr::null());
        let (mut id, mut ow, mut oh) = (0u64, 0u32, 0u32);
        let rc = unsafe { sys::infur_stream_collect_view(self.raw, &mut rgba, &mut sc, &mut id, &mut ow, &mut oh) };
        if rc != sys::INFUR_OK { return Err(HipError::from_ctx(&self.ctx, rc)); }
        let n = (ow as usize) * (oh as usize);
        // (a frame whose mask went straight to a caller-owned pinned buffer keeps no scaled copy: collect_view hands back NULL for it)
        let r = unsafe { std::slice::from_raw_parts(rgba, n * 4) };
        let s = if sc.is_null() { None } else { Some(unsafe { std::slice::from_raw_parts(sc, n * 3) }) };
        Ok(MaskView { stream: self, frame_id: id, size: [ow as usize, oh as usize], rgba: r, scaled_bgr: s })
    }
}
impl Drop for HipStream {
    fn drop(&mut self) { unsafe { sys::infur_stream_destroy(self.raw) } }
}
