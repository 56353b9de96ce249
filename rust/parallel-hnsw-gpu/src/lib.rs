//! `GpuComparator` and `GpuHnsw`: the reference crate's `Comparator` / `Hnsw` surface
//! (parallel-hnsw `src/lib.rs:53-74, 585-1686`) with every batch of distance evaluations and every
//! greedy layer search running in libphnsw's gfx950 kernels.  Method names, argument meaning and
//! result ordering follow the crate; what the crate does per element through Rayon
//! (`lib.rs:1107-1117, 2169-2184`) is one launch here.
//!
//! Written against `include/phnsw.h` through `phnsw-sys`; not compiled in this repository's build
//! image (no Rust toolchain).  `tests/test_rust_shim.py` checks every `phnsw_*` call made here
//! against the header (name and argument count).
use std::ffi::{CStr, CString};
use std::os::raw::{c_char, c_int, c_void};
use std::path::Path;
use std::sync::Arc;

use parallel_hnsw::parameters::{BuildParameters, OptimizationParameters, SearchParameters};
use parallel_hnsw::progress::{ProgressMonitor, ProgressUpdate};
use parallel_hnsw::{AbstractVector, Comparator, Layer, NodeId, VectorId};
use phnsw_sys as sys;

fn check(rc: c_int) {
    if rc != 0 {
        // the crate panics where this library returns a status (lib.rs:261,683,837; types.rs:86)
        let msg = unsafe { CStr::from_ptr(sys::phnsw_last_error()) }.to_string_lossy().into_owned();
        panic!("phnsw error {rc}: {msg}");
    }
}

fn sp_c(s: SearchParameters) -> sys::phnsw_search_params {
    sys::phnsw_search_params {
        number_of_candidates: s.number_of_candidates as u64,
        upper_layer_candidate_count: s.upper_layer_candidate_count as u64,
        probe_depth: s.probe_depth as u64,
    }
}
/// the sets of a batch in CSR form, as the calls by set take them; panics, naming `call`, unless `want` has one set per
/// query and at most 2^31 - 2 labels in all
fn pack_label_sets(want: &[Vec<u32>], nq: usize, call: &str) -> (Vec<u32>, Vec<u32>) {
    assert!(want.len() == nq, "{call}: one set of wanted labels per query");
    let mut first: Vec<u32> = Vec::with_capacity(nq + 1);
    let mut values: Vec<u32> = Vec::new();
    first.push(0);
    for s in want {
        values.extend_from_slice(s);
        assert!(values.len() <= 0x7FFF_FFFE, "{call}: too many wanted labels");
        first.push(values.len() as u32);
    }
    (first, values)
}
fn op_c(o: OptimizationParameters) -> sys::phnsw_optimization_params {
    sys::phnsw_optimization_params {
        promotion_threshold: o.promotion_threshold,
        neighborhood_threshold: o.neighborhood_threshold,
        recall_proportion: o.recall_proportion,
        promotion_proportion: o.promotion_proportion,
        search: sp_c(o.search),
    }
}
/// parameters.rs:42-64 field for field; seed / max_link_rounds / promote are libphnsw's additions
/// (`thread_rng` of lib.rs:832, the unbounded loop of lib.rs:1527, promote_at_layer on/off)
fn bp_c(bp: BuildParameters, seed: u64) -> sys::phnsw_build_params {
    sys::phnsw_build_params {
        order: bp.order as u64,
        zero_layer_neighborhood_size: bp.zero_layer_neighborhood_size as u64,
        neighborhood_size: bp.neighborhood_size as u64,
        optimization: op_c(bp.optimization),
        initial_partition_search: sp_c(bp.initial_partition_search),
        seed,
        max_link_rounds: 0,
        promote: 1,
    }
}

struct StoreHandle(*mut sys::phnsw_store);
unsafe impl Send for StoreHandle {}
unsafe impl Sync for StoreHandle {}
impl Drop for StoreHandle {
    fn drop(&mut self) {
        unsafe { sys::phnsw_store_destroy(self.0) }
    }
}

/// `BigComparator` (bigvec.rs:38-57) with its vectors also resident in HBM.  The scalar
/// `compare_raw` stays available on the host copy; batches go to the GPU.
#[derive(Clone)]
pub struct GpuComparator {
    host: Arc<Vec<Vec<f32>>>,
    store: Arc<StoreHandle>,
}

impl GpuComparator {
    pub fn new(data: Arc<Vec<Vec<f32>>>, device: i32) -> Self {
        let dim = data[0].len();
        let mut flat: Vec<f32> = Vec::with_capacity(data.len() * dim);
        for v in data.iter() {
            assert_eq!(v.len(), dim);
            flat.extend_from_slice(v);
        }
        let mut s = std::ptr::null_mut();
        check(unsafe {
            sys::phnsw_store_create(flat.as_ptr(), data.len() as u64, dim as u32, sys::PHNSW_METRIC_COSINE_HALF,
                                    device, &mut s)
        });
        GpuComparator { host: data, store: Arc::new(StoreHandle(s)) }
    }

    /// The same vectors with their HBM rows rounded to IEEE half floats (`phnsw_store_create_f16`): half the bytes per
    /// gathered candidate.  Search-only -- adopt a graph built over the f32 comparator with `GpuHnsw::from_layers`
    /// and re-rank with `GpuHnsw::search_many_reranked`.  The host copy (and `compare_raw`) stays f32.
    pub fn to_f16(&self) -> Self {
        let mut s = std::ptr::null_mut();
        check(unsafe { sys::phnsw_store_create_f16(self.store.0, &mut s) });
        GpuComparator { host: self.host.clone(), store: Arc::new(StoreHandle(s)) }
    }

    /// The same vectors with their HBM rows scalar-quantised to int8, one f32 scale per row (`phnsw_store_create_i8`): a
    /// quarter of the bytes per gathered candidate.  Search-only, like `to_f16()`; re-rank with
    /// `GpuHnsw::search_many_reranked_i8`.  The host copy (and `compare_raw`) stays f32.
    pub fn to_i8(&self) -> Self {
        let mut s = std::ptr::null_mut();
        check(unsafe { sys::phnsw_store_create_i8(self.store.0, &mut s) });
        GpuComparator { host: self.host.clone(), store: Arc::new(StoreHandle(s)) }
    }

    /// The rows of `to_i8()`, searched with an int8 query and integer dot products (`phnsw_store_create_i8q`):
    /// dot-product metrics only.  Search-only; re-rank with `GpuHnsw::search_many_reranked_i8q`.
    pub fn to_i8q(&self) -> Self {
        let mut s = std::ptr::null_mut();
        check(unsafe { sys::phnsw_store_create_i8q(self.store.0, &mut s) });
        GpuComparator { host: self.host.clone(), store: Arc::new(StoreHandle(s)) }
    }

    /// The same vectors as one sign bit per component (`phnsw_store_create_bits`): Hamming distances in sign-vector
    /// units, plain searches only.  Re-rank with `GpuHnsw::search_many_reranked_bits` for true f32 distances.
    pub fn to_bits(&self) -> Self {
        let mut s = std::ptr::null_mut();
        check(unsafe { sys::phnsw_store_create_bits(self.store.0, &mut s) });
        GpuComparator { host: self.host.clone(), store: Arc::new(StoreHandle(s)) }
    }

    /// the sign bits `[n][ceil(dim / 32)]` of a `to_bits()` comparator (`phnsw_bits_read`)
    pub fn bits_words(&self) -> Vec<u32> {
        let (n, dim) = (self.host.len(), self.host.first().map_or(0, |v| v.len()));
        let mut words = vec![0u32; n * ((dim + 31) / 32)];
        check(unsafe { sys::phnsw_bits_read(self.store.0, words.as_mut_ptr()) });
        words
    }

    /// codes `[n][dim]` and scales `[n]` of a `to_i8()` or `to_i8q()` comparator (`phnsw_i8_read`)
    pub fn i8_codes_and_scales(&self) -> (Vec<i8>, Vec<f32>) {
        let (n, dim) = (self.host.len(), self.host.first().map_or(0, |v| v.len()));
        let (mut codes, mut scales) = (vec![0i8; n * dim], vec![0f32; n]);
        check(unsafe { sys::phnsw_i8_read(self.store.0, codes.as_mut_ptr(), scales.as_mut_ptr()) });
        (codes, scales)
    }

    /// `compare_vec(v, Stored(id))` for a whole candidate list in one launch (lib.rs:69-73)
    pub fn compare_batch(&self, v: AbstractVector<Vec<f32>>, ids: &[VectorId]) -> Vec<f32> {
        let raw: Vec<u64> = ids.iter().map(|i| i.0 as u64).collect();
        let mut out = vec![0f32; ids.len()];
        let rc = unsafe {
            match v {
                AbstractVector::Stored(q) => sys::phnsw_distance_batch(self.store.0, std::ptr::null(), q.0 as u64,
                                                                       raw.as_ptr(), raw.len() as u64, out.as_mut_ptr()),
                AbstractVector::Unstored(q) => sys::phnsw_distance_batch(self.store.0, q.as_ptr(), 0, raw.as_ptr(),
                                                                         raw.len() as u64, out.as_mut_ptr()),
            }
        };
        check(rc);
        out
    }
}

impl Comparator for GpuComparator {
    type T = Vec<f32>;
    type Borrowable<'a> = &'a Vec<f32>;
    fn lookup(&self, v: VectorId) -> &Vec<f32> {
        &self.host[v.0]
    }
    fn compare_raw(&self, v1: &Vec<f32>, v2: &Vec<f32>) -> f32 {
        // bigvec.rs:47-53
        let mut result = 0.0;
        for (&f1, &f2) in v1.iter().zip(v2.iter()) {
            result += f1 * f2
        }
        (1.0 - result) / 2.0
    }
}

unsafe extern "C" fn progress_trampoline(user: *mut c_void, phase: *const c_char, done: u64, total: u64) -> c_int {
    let monitor = &mut *(user as *mut &mut dyn ProgressMonitor);
    let phase = CStr::from_ptr(phase).to_string_lossy();
    let state = serde_json::json!({ "phase": phase, "done": done, "total": total });
    match monitor.update(ProgressUpdate { state }) {
        Ok(()) => 0,
        Err(_) => 1, // Interrupt (progress.rs:8-10)
    }
}

/// `Hnsw<GpuComparator>` whose layers live on the GPU.
/// The collective seam of the sharded build (`phnsw_comm`): the library's own RCCL transport over xGMI -- rank 0
/// makes the 128-byte id, the host hands it to the other ranks (a file, MPI, a socket), every rank creates its
/// communicator on its own GPU -- or any transport the host supplies as two callbacks.
pub struct ShardComm {
    owned: *mut sys::phnsw_comm,
    custom: Option<Box<sys::phnsw_comm>>,
}
unsafe impl Send for ShardComm {}
impl ShardComm {
    pub fn rccl_unique_id() -> [u8; 128] {
        let mut id = [0u8; 128];
        check(unsafe { sys::phnsw_comm_rccl_unique_id(id.as_mut_ptr()) });
        id
    }
    pub fn rccl(id: &[u8; 128], rank: u32, world: u32, device: i32) -> Self {
        let mut c = std::ptr::null_mut();
        check(unsafe { sys::phnsw_comm_rccl_create(id.as_ptr(), rank, world, device, &mut c) });
        ShardComm { owned: c, custom: None }
    }
    /// a transport of the host's own (MPI, ...): see `phnsw_comm` in include/phnsw.h for the two callbacks
    pub fn custom(c: sys::phnsw_comm) -> Self {
        ShardComm { owned: std::ptr::null_mut(), custom: Some(Box::new(c)) }
    }
    /// every rank calls it: a known pattern through the all-gather and the all-reduce, verified on every rank
    pub fn selftest(&self, bytes: u64) {
        check(unsafe { sys::phnsw_comm_selftest(self.as_ptr(), bytes) });
    }
    fn as_ptr(&self) -> *const sys::phnsw_comm {
        match &self.custom {
            Some(b) => &**b as *const sys::phnsw_comm,
            None => self.owned as *const sys::phnsw_comm,
        }
    }
}
impl Drop for ShardComm {
    fn drop(&mut self) {
        if !self.owned.is_null() {
            unsafe { sys::phnsw_comm_destroy(self.owned) }
        }
    }
}

pub struct GpuHnsw {
    ix: *mut sys::phnsw_index,
    comparator: GpuComparator,
    pub build_parameters: BuildParameters,
}
unsafe impl Send for GpuHnsw {}
unsafe impl Sync for GpuHnsw {} // search entry points are thread safe (phnsw.h)

impl Drop for GpuHnsw {
    fn drop(&mut self) {
        unsafe { sys::phnsw_index_destroy(self.ix) }
    }
}

/// `phnsw_labels`: the posting lists of a label column (`GpuHnsw::labels`).  Must not be used after its index is dropped
pub struct GpuLabels {
    lb: *mut sys::phnsw_labels,
}
unsafe impl Send for GpuLabels {}
unsafe impl Sync for GpuLabels {} // the search calls keep a scratch set per call in flight with the handle (phnsw.h)

impl Drop for GpuLabels {
    fn drop(&mut self) {
        unsafe { sys::phnsw_labels_destroy(self.lb) } // waits for the calls in flight that use it
    }
}

impl GpuLabels {
    /// (distinct labels that list a vector, listed vectors, the longest list)
    pub fn info(&self) -> (u64, u64, u64) {
        let (mut n, mut nlabels, mut listed, mut longest) = (0u64, 0u64, 0u64, 0u64);
        check(unsafe { sys::phnsw_labels_info(self.lb, &mut n, &mut nlabels, &mut listed, &mut longest) });
        (nlabels, listed, longest)
    }

    /// per query the length of the list of `want_dev[q]` (`phnsw_labels_count_device`)
    ///
    /// # Safety
    /// `want_dev` and `out_count_dev` (`nq` u32 each) must be valid device allocations
    pub unsafe fn count_device(&self, want_dev: *const u32, nq: u64, out_count_dev: *mut u32, stream: *mut c_void) {
        check(sys::phnsw_labels_count_device(self.lb, want_dev, nq, out_count_dev, stream));
    }

    /// per query the summed list lengths of the distinct labels of its set (`phnsw_labels_count_set_device`); the sets
    /// in CSR form
    ///
    /// # Safety
    /// `want_first_dev` (`nq + 1` u32), `want_values_dev` (`nwant` u32) and `out_count_dev` (`nq` u32) must be valid
    /// device allocations
    pub unsafe fn count_set_device(&self, want_first_dev: *const u32, want_values_dev: *const u32, nq: u64, nwant: u64,
                                   out_count_dev: *mut u32, stream: *mut c_void) {
        check(sys::phnsw_labels_count_set_device(self.lb, want_first_dev, want_values_dev, nq, nwant, out_count_dev, stream));
    }
}

impl GpuHnsw {
    /// `Hnsw::generate(c, vs, bp, progress)`  lib.rs:825-830
    pub fn generate(c: GpuComparator, vs: Vec<VectorId>, bp: BuildParameters, progress: &mut dyn ProgressMonitor) -> Self {
        let raw: Vec<u64> = vs.iter().map(|v| v.0 as u64).collect();
        let mut ix = std::ptr::null_mut();
        let mut monitor: &mut dyn ProgressMonitor = progress;
        check(unsafe {
            sys::phnsw_build(c.store.0, raw.as_ptr(), raw.len() as u64, &bp_c(bp, 0), Some(progress_trampoline),
                             &mut monitor as *mut &mut dyn ProgressMonitor as *mut c_void, &mut ix)
        });
        GpuHnsw { ix, comparator: c, build_parameters: bp }
    }

    /// `Hnsw::generate` with every per-node phase split over the GPUs of one node (BASELINE config 4): one process
    /// per GPU, every rank calls this with the same vectors, ids and parameters and ends with the same index
    /// (`phnsw_build_sharded`: node ranges per round, all-gather of the per-node results, lib.rs:1097-1153)
    pub fn generate_sharded(c: GpuComparator, vs: Vec<VectorId>, bp: BuildParameters, comm: &ShardComm,
                            progress: &mut dyn ProgressMonitor) -> (Self, sys::phnsw_sharded_stats) {
        let raw: Vec<u64> = vs.iter().map(|v| v.0 as u64).collect();
        let mut ix = std::ptr::null_mut();
        let mut stats = sys::phnsw_sharded_stats::default();
        let mut monitor: &mut dyn ProgressMonitor = progress;
        check(unsafe {
            sys::phnsw_build_sharded(c.store.0, raw.as_ptr(), raw.len() as u64, &bp_c(bp, 0), comm.as_ptr(),
                                     Some(progress_trampoline), &mut monitor as *mut &mut dyn ProgressMonitor as *mut c_void,
                                     &mut ix, &mut stats)
        });
        (GpuHnsw { ix, comparator: c, build_parameters: bp }, stats)
    }

    /// adopt the layers of an `Hnsw` the crate built or deserialised (top first, lib.rs:587)
    pub fn from_layers(c: GpuComparator, layers: &[Layer<GpuComparator>], bp: BuildParameters) -> Self {
        let counts: Vec<u64> = layers.iter().map(|l| l.nodes.len() as u64).collect();
        let widths: Vec<u64> = layers.iter().map(|l| l.neighborhood_size as u64).collect();
        let nodes: Vec<Vec<u64>> = layers.iter().map(|l| l.nodes.iter().map(|v| v.0 as u64).collect()).collect();
        let nbrs: Vec<Vec<u64>> = layers.iter().map(|l| l.neighbors.iter().map(|n| n.0 as u64).collect()).collect();
        let np: Vec<*const u64> = nodes.iter().map(|v| v.as_ptr()).collect();
        let bp_: Vec<*const u64> = nbrs.iter().map(|v| v.as_ptr()).collect();
        let mut ix = std::ptr::null_mut();
        check(unsafe {
            sys::phnsw_index_from_layers(c.store.0, layers.len() as u32, counts.as_ptr(), widths.as_ptr(), np.as_ptr(),
                                         bp_.as_ptr(), &mut ix)
        });
        GpuHnsw { ix, comparator: c, build_parameters: bp }
    }

    pub fn comparator(&self) -> &GpuComparator {
        &self.comparator // lib.rs:648-650
    }
    pub fn layer_count(&self) -> usize {
        unsafe { sys::phnsw_index_layer_count(self.ix) as usize } // lib.rs:644-646
    }
    pub fn vector_count(&self) -> usize {
        let mut n = 0u64;
        check(unsafe {
            sys::phnsw_index_layer_info(self.ix, self.layer_count() as u32 - 1, &mut n, std::ptr::null_mut())
        });
        n as usize // lib.rs:592-594
    }

    /// `Layer { comparator, neighborhood_size, nodes, neighbors }` of layer `from_top` (lib.rs:85-91):
    /// what the crate's own `serialize` (serialize.rs:33-124) and diagnostics need
    pub fn layer(&self, from_top: usize) -> Layer<GpuComparator> {
        let (mut n, mut w) = (0u64, 0u64);
        check(unsafe { sys::phnsw_index_layer_info(self.ix, from_top as u32, &mut n, &mut w) });
        let (mut nodes, mut nbrs) = (vec![0u64; n as usize], vec![0u64; (n * w) as usize]);
        check(unsafe { sys::phnsw_index_layer_read(self.ix, from_top as u32, nodes.as_mut_ptr(), nbrs.as_mut_ptr()) });
        Layer {
            comparator: self.comparator.clone(),
            neighborhood_size: w as usize,
            nodes: nodes.into_iter().map(|v| VectorId(v as usize)).collect(),
            // u64::MAX == !0usize: the empty-slot sentinel survives the cast (types.rs:8-13)
            neighbors: nbrs.into_iter().map(|x| NodeId(x as usize)).collect(),
        }
    }

    /// `Hnsw::search(v, sp)`  lib.rs:663-665
    pub fn search(&self, v: AbstractVector<Vec<f32>>, sp: SearchParameters) -> Vec<(VectorId, f32)> {
        self.search_many(&[v], sp, 0).pop().unwrap()
    }
    /// `Hnsw::search_upto(v, sp, upto_layer_from_top)`  lib.rs:654-661
    pub fn search_upto(&self, v: AbstractVector<Vec<f32>>, sp: SearchParameters, upto: usize) -> Vec<(VectorId, f32)> {
        self.search_many(&[v], sp, upto as u32).pop().unwrap()
    }
    /// a batch of queries in one launch (what the crate's callers get from `par_iter().map(search)`,
    /// lib.rs:1107-1117, 2169-2184); all Stored or all Unstored
    pub fn search_many(&self, vs: &[AbstractVector<Vec<f32>>], sp: SearchParameters, upto: u32)
                       -> Vec<Vec<(VectorId, f32)>> {
        let (nq, ef) = (vs.len(), sp.number_of_candidates);
        let psp = sp_c(sp);
        let (mut ids, mut d, mut len) = (vec![0u64; nq * ef], vec![0f32; nq * ef], vec![0u64; nq]);
        let rc = match vs.first() {
            None => return Vec::new(),
            Some(AbstractVector::Stored(_)) => {
                let q: Vec<u64> = vs.iter().map(|v| match v {
                    AbstractVector::Stored(i) => i.0 as u64,
                    _ => panic!("search_many: mixed Stored / Unstored"),
                }).collect();
                unsafe {
                    sys::phnsw_search_batch_stored(self.ix, q.as_ptr(), nq as u64, &psp, upto, std::ptr::null(),
                                                   ids.as_mut_ptr(), d.as_mut_ptr(), len.as_mut_ptr(),
                                                   std::ptr::null_mut())
                }
            }
            Some(AbstractVector::Unstored(_)) => {
                let mut q: Vec<f32> = Vec::new();
                for v in vs {
                    match v {
                        AbstractVector::Unstored(x) => q.extend_from_slice(x),
                        _ => panic!("search_many: mixed Stored / Unstored"),
                    }
                }
                unsafe {
                    sys::phnsw_search_batch(self.ix, q.as_ptr(), nq as u64, &psp, upto, std::ptr::null(),
                                            ids.as_mut_ptr(), d.as_mut_ptr(), len.as_mut_ptr(), std::ptr::null_mut())
                }
            }
        };
        check(rc);
        (0..nq).map(|q| (0..len[q] as usize).map(|k| (VectorId(ids[q * ef + k] as usize), d[q * ef + k])).collect())
               .collect()
    }

    /// `search(v, sp)` for a batch of raw queries keeping the best `k` of each: the truncation the crate's callers do
    /// themselves (lib.rs:1118) happens on the device, before the transfer (`phnsw_search_batch_topk`)
    pub fn search_many_topk(&self, queries: &[Vec<f32>], sp: SearchParameters, k: usize) -> Vec<Vec<(VectorId, f32)>> {
        let nq = queries.len();
        let psp = sp_c(sp);
        let mut q: Vec<f32> = Vec::with_capacity(nq * queries.first().map_or(0, |x| x.len()));
        for x in queries {
            q.extend_from_slice(x);
        }
        let (mut ids, mut d, mut len) = (vec![0u64; nq * k], vec![0f32; nq * k], vec![0u64; nq]);
        check(unsafe {
            sys::phnsw_search_batch_topk(self.ix, q.as_ptr(), std::ptr::null(), nq as u64, &psp, 0, std::ptr::null(), k as u64,
                                         ids.as_mut_ptr(), d.as_mut_ptr(), len.as_mut_ptr())
        });
        (0..nq).map(|i| (0..len[i] as usize).map(|j| (VectorId(ids[i * k + j] as usize), d[i * k + j])).collect()).collect()
    }

    /// `search_many_topk` restricted to the VectorIds `include` accepts: `Layer::closest_vectors`' closure
    /// (lib.rs:250-277) evaluated once per id into an allow bitmap shared by the batch (`phnsw_search_batch_filtered`).
    /// A post-filter on each layer's queue: expect about density * number_of_candidates results.  The entry vector can
    /// come back although `include` rejects it, as in the reference; `strict` removes it.  `k` 0 = all
    /// `number_of_candidates` entries of a row; panics on `k > number_of_candidates`
    pub fn search_many_filtered<F: Fn(VectorId) -> bool>(&self, queries: &[Vec<f32>], sp: SearchParameters, k: usize,
                                                         include: F, strict: bool) -> Vec<Vec<(VectorId, f32)>> {
        let nq = queries.len();
        // the C call reads k 0 as "the whole row": the buffers below are sized by the k it will write
        let k = if k == 0 { sp.number_of_candidates } else { k };
        assert!(k <= sp.number_of_candidates, "search_many_filtered: k exceeds number_of_candidates");
        let psp = sp_c(sp);
        let mut n64 = 0u64;
        check(unsafe {
            sys::phnsw_store_info(self.comparator.store.0, &mut n64, std::ptr::null_mut(), std::ptr::null_mut(),
                                  std::ptr::null_mut(), std::ptr::null_mut())
        });
        let n = n64 as usize; // the bitmap covers every VectorId of the store
        let mut words = vec![0u32; (n + 31) / 32];
        for v in 0..n {
            if include(VectorId(v)) {
                words[v >> 5] |= 1u32 << (v & 31);
            }
        }
        let mut q: Vec<f32> = Vec::with_capacity(nq * queries.first().map_or(0, |x| x.len()));
        for x in queries {
            q.extend_from_slice(x);
        }
        let (mut ids, mut d, mut len) = (vec![0u64; nq * k], vec![0f32; nq * k], vec![0u64; nq]);
        check(unsafe {
            sys::phnsw_search_batch_filtered(self.ix, q.as_ptr(), std::ptr::null(), nq as u64, &psp, 0, std::ptr::null(),
                                             words.as_ptr(), 0, if strict { sys::PHNSW_FILTER_STRICT } else { 0 }, k as u64,
                                             ids.as_mut_ptr(), d.as_mut_ptr(), len.as_mut_ptr(), std::ptr::null_mut())
        });
        (0..nq).map(|i| (0..len[i] as usize).map(|j| (VectorId(ids[i * k + j] as usize), d[i * k + j])).collect()).collect()
    }

    /// zero-copy form (`phnsw_search_batch_filtered_device`): `filter_dev` holds one bitmap (`filter_stride_words` 0)
    /// or one per query; null = the default set with `set_filter_device`
    ///
    /// # Safety
    /// the pointers must be valid device allocations of the sizes `phnsw.h` documents for the call
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn search_filtered_device(&self, queries_dev: *const f32, ldq: u32, qids_dev: *const u32, nq: u64,
                                         sp: SearchParameters, upto: u32, exclude_dev: *const u32, filter_dev: *const u32,
                                         filter_stride_words: u32, strict: bool, out_ids_dev: *mut u32, out_d_dev: *mut f32,
                                         out_len_dev: *mut u32, out_stats_dev: *mut u32, status_dev: *mut u32,
                                         stream: *mut c_void) {
        let psp = sp_c(sp);
        check(sys::phnsw_search_batch_filtered_device(self.ix, queries_dev, ldq, qids_dev, nq, &psp, upto, exclude_dev, filter_dev,
                                                      filter_stride_words, if strict { sys::PHNSW_FILTER_STRICT } else { 0 },
                                                      out_ids_dev, out_d_dev, out_len_dev, out_stats_dev, status_dev, stream));
    }

    /// tombstones (`phnsw_index_set_filter_device`): a shared device bitmap the caller keeps alive becomes the filter
    /// of every filtered call that passes none; null clears it.  Not while searches are in flight
    ///
    /// # Safety
    /// `filter_dev` must stay a valid device allocation of ceil(n / 32) words until it is cleared
    pub unsafe fn set_filter_device(&mut self, filter_dev: *const u32) {
        check(sys::phnsw_index_set_filter_device(self.ix, filter_dev));
    }

    /// the exact `k` nearest among the VectorIds `include` accepts (`phnsw_search_exact_filtered`): the allowed rows are
    /// scanned instead of the graph walked, so the recall is 1 -- the call for selective filters, where
    /// `search_many_filtered` returns about density * number_of_candidates results.  Only vectors of the index are
    /// candidates, a rejected id is never returned, results ascend by (distance, id).  Panics unless 1 <= k <= 1024
    pub fn search_many_exact_filtered<F: Fn(VectorId) -> bool>(&self, queries: &[Vec<f32>], k: usize, include: F)
                                                               -> Vec<Vec<(VectorId, f32)>> {
        assert!((1..=1024).contains(&k), "search_many_exact_filtered: k must be 1..1024");
        let nq = queries.len();
        let mut n64 = 0u64;
        check(unsafe {
            sys::phnsw_store_info(self.comparator.store.0, &mut n64, std::ptr::null_mut(), std::ptr::null_mut(),
                                  std::ptr::null_mut(), std::ptr::null_mut())
        });
        let n = n64 as usize;
        let mut words = vec![0u32; (n + 31) / 32];
        for v in 0..n {
            if include(VectorId(v)) {
                words[v >> 5] |= 1u32 << (v & 31);
            }
        }
        let mut q: Vec<f32> = Vec::with_capacity(nq * queries.first().map_or(0, |x| x.len()));
        for x in queries {
            q.extend_from_slice(x);
        }
        let (mut ids, mut d, mut len) = (vec![0u64; nq * k], vec![0f32; nq * k], vec![0u64; nq]);
        check(unsafe {
            sys::phnsw_search_exact_filtered(self.ix, q.as_ptr(), std::ptr::null(), nq as u64, std::ptr::null(), words.as_ptr(),
                                             0, k as u64, ids.as_mut_ptr(), d.as_mut_ptr(), len.as_mut_ptr())
        });
        (0..nq).map(|i| (0..len[i] as usize).map(|j| (VectorId(ids[i * k + j] as usize), d[i * k + j])).collect()).collect()
    }

    /// zero-copy form (`phnsw_search_exact_filtered_device`): u32 ids `[nq][k]`, enqueued on `stream`
    ///
    /// # Safety
    /// the pointers must be valid device allocations of the sizes `phnsw.h` documents for the call
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn search_exact_filtered_device(&self, queries_dev: *const f32, ldq: u32, qids_dev: *const u32, nq: u64,
                                               exclude_dev: *const u32, filter_dev: *const u32, filter_stride_words: u32,
                                               k: u64, out_ids_dev: *mut u32, out_d_dev: *mut f32, out_len_dev: *mut u32,
                                               status_dev: *mut u32, stream: *mut c_void) {
        check(sys::phnsw_search_exact_filtered_device(self.ix, queries_dev, ldq, qids_dev, nq, exclude_dev, filter_dev,
                                                      filter_stride_words, k, out_ids_dev, out_d_dev, out_len_dev, status_dev,
                                                      stream));
    }

    /// `search_many_exact_filtered` computed as a queries x candidates distance table (`phnsw_search_exact_shared`):
    /// `include` is one predicate for the whole batch, so every query meets the same rows.  The same results, bit for
    /// bit.  f32, f16, i8 and i8q stores with rows up to 1536 floats.  Panics unless 1 <= k <= 1024
    pub fn search_many_exact_shared<F: Fn(VectorId) -> bool>(&self, queries: &[Vec<f32>], k: usize, include: F)
                                                             -> Vec<Vec<(VectorId, f32)>> {
        assert!((1..=1024).contains(&k), "search_many_exact_shared: k must be 1..1024");
        let nq = queries.len();
        let mut n64 = 0u64;
        check(unsafe {
            sys::phnsw_store_info(self.comparator.store.0, &mut n64, std::ptr::null_mut(), std::ptr::null_mut(),
                                  std::ptr::null_mut(), std::ptr::null_mut())
        });
        let n = n64 as usize;
        let mut words = vec![0u32; (n + 31) / 32];
        for v in 0..n {
            if include(VectorId(v)) {
                words[v >> 5] |= 1u32 << (v & 31);
            }
        }
        let mut q: Vec<f32> = Vec::with_capacity(nq * queries.first().map_or(0, |x| x.len()));
        for x in queries {
            q.extend_from_slice(x);
        }
        let (mut ids, mut d, mut len) = (vec![0u64; nq * k], vec![0f32; nq * k], vec![0u64; nq]);
        check(unsafe {
            sys::phnsw_search_exact_shared(self.ix, q.as_ptr(), std::ptr::null(), nq as u64, std::ptr::null(), words.as_ptr(),
                                           k as u64, ids.as_mut_ptr(), d.as_mut_ptr(), len.as_mut_ptr())
        });
        (0..nq).map(|i| (0..len[i] as usize).map(|j| (VectorId(ids[i * k + j] as usize), d[i * k + j])).collect()).collect()
    }

    /// zero-copy form (`phnsw_search_exact_shared_device`): u32 ids `[nq][k]`; synchronises `stream` once
    ///
    /// # Safety
    /// the pointers must be valid device allocations of the sizes `phnsw.h` documents for the call
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn search_exact_shared_device(&self, queries_dev: *const f32, ldq: u32, qids_dev: *const u32, nq: u64,
                                             exclude_dev: *const u32, filter_dev: *const u32, k: u64,
                                             out_ids_dev: *mut u32, out_d_dev: *mut f32, out_len_dev: *mut u32,
                                             status_dev: *mut u32, stream: *mut c_void) {
        check(sys::phnsw_search_exact_shared_device(self.ix, queries_dev, ldq, qids_dev, nq, exclude_dev, filter_dev, k,
                                                    out_ids_dev, out_d_dev, out_len_dev, status_dev, stream));
    }

    /// `search_many_exact_filtered` for a table of predicates and a selector per query (`phnsw_search_exact_grouped`):
    /// query i may return the vectors `includes[include_of[i]]` accepts, every vector of the index when `include_of[i]`
    /// is `None`.  The batch is grouped by predicate on the device and every group runs as `search_many_exact_shared`
    /// runs its batch: the same results, bit for bit.  Panics unless 1 <= k <= 1024, `includes` is not empty,
    /// `include_of` has one entry per query and every selector names a predicate
    pub fn search_many_exact_grouped<F: Fn(VectorId) -> bool>(&self, queries: &[Vec<f32>], k: usize, includes: &[F],
                                                              include_of: &[Option<usize>])
                                                              -> Vec<Vec<(VectorId, f32)>> {
        assert!((1..=1024).contains(&k), "search_many_exact_grouped: k must be 1..1024");
        assert!(!includes.is_empty(), "search_many_exact_grouped: an empty table of predicates");
        let nq = queries.len();
        assert!(include_of.len() == nq, "search_many_exact_grouped: one selector per query");
        assert!(include_of.iter().all(|s| s.map_or(true, |i| i < includes.len())),
                "search_many_exact_grouped: a selector outside the table");
        let mut n64 = 0u64;
        check(unsafe {
            sys::phnsw_store_info(self.comparator.store.0, &mut n64, std::ptr::null_mut(), std::ptr::null_mut(),
                                  std::ptr::null_mut(), std::ptr::null_mut())
        });
        let n = n64 as usize;
        let stride = (n + 31) / 32;
        let mut words = vec![0u32; includes.len() * stride];
        for (f, include) in includes.iter().enumerate() {
            for v in 0..n {
                if include(VectorId(v)) {
                    words[f * stride + (v >> 5)] |= 1u32 << (v & 31);
                }
            }
        }
        let of: Vec<u32> = include_of.iter().map(|s| s.map_or(sys::PHNSW_FILTER_ALL, |i| i as u32)).collect();
        let mut q: Vec<f32> = Vec::with_capacity(nq * queries.first().map_or(0, |x| x.len()));
        for x in queries {
            q.extend_from_slice(x);
        }
        let (mut ids, mut d, mut len) = (vec![0u64; nq * k], vec![0f32; nq * k], vec![0u64; nq]);
        check(unsafe {
            sys::phnsw_search_exact_grouped(self.ix, q.as_ptr(), std::ptr::null(), nq as u64, std::ptr::null(), words.as_ptr(),
                                            stride as u32, includes.len() as u64, of.as_ptr(), k as u64, ids.as_mut_ptr(),
                                            d.as_mut_ptr(), len.as_mut_ptr())
        });
        (0..nq).map(|i| (0..len[i] as usize).map(|j| (VectorId(ids[i * k + j] as usize), d[i * k + j])).collect()).collect()
    }

    /// zero-copy form (`phnsw_search_exact_grouped_device`): u32 ids `[nq][k]`; synchronises `stream` once
    ///
    /// # Safety
    /// the pointers must be valid device allocations of the sizes `phnsw.h` documents for the call
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn search_exact_grouped_device(&self, queries_dev: *const f32, ldq: u32, qids_dev: *const u32, nq: u64,
                                              exclude_dev: *const u32, filters_dev: *const u32, filter_stride_words: u32,
                                              nfilters: u64, filter_of_dev: *const u32, k: u64, out_ids_dev: *mut u32,
                                              out_d_dev: *mut f32, out_len_dev: *mut u32, status_dev: *mut u32,
                                              stream: *mut c_void) {
        check(sys::phnsw_search_exact_grouped_device(self.ix, queries_dev, ldq, qids_dev, nq, exclude_dev, filters_dev,
                                                     filter_stride_words, nfilters, filter_of_dev, k, out_ids_dev, out_d_dev,
                                                     out_len_dev, status_dev, stream));
    }

    /// one label per vector of the store, turned once into posting lists on the device (`phnsw_labels_create`):
    /// `labels[v]` is the label of vector v, `None` = not listed.  A snapshot: after the store or the index has changed
    /// `search_many_exact_labeled` refuses it as stale.  Panics unless `labels` has one entry per vector
    pub fn labels(&self, labels: &[Option<u32>]) -> GpuLabels {
        let col: Vec<u32> = labels.iter().map(|l| l.unwrap_or(sys::PHNSW_LABEL_NONE)).collect();
        let mut lb: *mut sys::phnsw_labels = std::ptr::null_mut();
        check(unsafe { sys::phnsw_labels_create(self.ix, col.as_ptr(), col.len() as u64, &mut lb) });
        GpuLabels { lb }
    }

    /// `search_many_exact_filtered` by row label (`phnsw_search_exact_labeled`): query i may return the vectors `labels`
    /// lists under `want[i]`; `None`, or a label nobody carries, gives an empty result.  The same results, bit for bit,
    /// as the predicates `label of v == want[i]` give, from posting lists instead of bitmaps.  Panics unless
    /// 1 <= k <= 1024 and `want` has one entry per query
    pub fn search_many_exact_labeled(&self, queries: &[Vec<f32>], k: usize, labels: &GpuLabels, want: &[Option<u32>])
                                     -> Vec<Vec<(VectorId, f32)>> {
        assert!((1..=1024).contains(&k), "search_many_exact_labeled: k must be 1..1024");
        let nq = queries.len();
        assert!(want.len() == nq, "search_many_exact_labeled: one wanted label per query");
        let w: Vec<u32> = want.iter().map(|l| l.unwrap_or(sys::PHNSW_LABEL_NONE)).collect();
        let mut q: Vec<f32> = Vec::with_capacity(nq * queries.first().map_or(0, |x| x.len()));
        for x in queries {
            q.extend_from_slice(x);
        }
        let (mut ids, mut d, mut len) = (vec![0u64; nq * k], vec![0f32; nq * k], vec![0u64; nq]);
        check(unsafe {
            sys::phnsw_search_exact_labeled(self.ix, labels.lb, q.as_ptr(), std::ptr::null(), nq as u64, std::ptr::null(),
                                            w.as_ptr(), k as u64, ids.as_mut_ptr(), d.as_mut_ptr(), len.as_mut_ptr())
        });
        (0..nq).map(|i| (0..len[i] as usize).map(|j| (VectorId(ids[i * k + j] as usize), d[i * k + j])).collect()).collect()
    }

    /// zero-copy form (`phnsw_search_exact_labeled_device`): u32 ids `[nq][k]`; enqueued on `stream`, never synchronises it
    ///
    /// # Safety
    /// the pointers must be valid device allocations of the sizes `phnsw.h` documents for the call
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn search_exact_labeled_device(&self, labels: &GpuLabels, queries_dev: *const f32, ldq: u32,
                                              qids_dev: *const u32, nq: u64, exclude_dev: *const u32, want_dev: *const u32,
                                              k: u64, out_ids_dev: *mut u32, out_d_dev: *mut f32, out_len_dev: *mut u32,
                                              status_dev: *mut u32, stream: *mut c_void) {
        check(sys::phnsw_search_exact_labeled_device(self.ix, labels.lb, queries_dev, ldq, qids_dev, nq, exclude_dev, want_dev, k,
                                                     out_ids_dev, out_d_dev, out_len_dev, status_dev, stream));
    }

    /// `search_many_exact_labeled` for a set of labels per query (`phnsw_search_exact_labelset`): query i may return the
    /// vectors `labels` lists under any label of `want[i]`; an empty set and labels nobody carries give nothing, a label
    /// twice counts once.  The same results, bit for bit, as the predicates `label of v in want[i]` give.  The exact
    /// scan; `search_many_labelset` walks the graph by set, `search_many_labelset_auto` routes.  Panics unless 1 <= k <= 1024 and `want` has one set per query
    pub fn search_many_exact_labelset(&self, queries: &[Vec<f32>], k: usize, labels: &GpuLabels, want: &[Vec<u32>])
                                      -> Vec<Vec<(VectorId, f32)>> {
        assert!((1..=1024).contains(&k), "search_many_exact_labelset: k must be 1..1024");
        let nq = queries.len();
        let (first, values) = pack_label_sets(want, nq, "search_many_exact_labelset");
        let mut q: Vec<f32> = Vec::with_capacity(nq * queries.first().map_or(0, |x| x.len()));
        for x in queries {
            q.extend_from_slice(x);
        }
        let (mut ids, mut d, mut len) = (vec![0u64; nq * k], vec![0f32; nq * k], vec![0u64; nq]);
        check(unsafe {
            sys::phnsw_search_exact_labelset(self.ix, labels.lb, q.as_ptr(), std::ptr::null(), nq as u64, std::ptr::null(),
                                             first.as_ptr(), values.as_ptr(), k as u64, ids.as_mut_ptr(), d.as_mut_ptr(),
                                             len.as_mut_ptr())
        });
        (0..nq).map(|i| (0..len[i] as usize).map(|j| (VectorId(ids[i * k + j] as usize), d[i * k + j])).collect()).collect()
    }

    /// zero-copy form (`phnsw_search_exact_labelset_device`): the sets in CSR form; status 8 = a range of
    /// `want_first_dev` that is not sound; enqueued on `stream`, never synchronises it
    ///
    /// # Safety
    /// the pointers must be valid device allocations of the sizes `phnsw.h` documents for the call
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn search_exact_labelset_device(&self, labels: &GpuLabels, queries_dev: *const f32, ldq: u32,
                                               qids_dev: *const u32, nq: u64, exclude_dev: *const u32,
                                               want_first_dev: *const u32, want_values_dev: *const u32, nwant: u64, k: u64,
                                               out_ids_dev: *mut u32, out_d_dev: *mut f32, out_len_dev: *mut u32,
                                               status_dev: *mut u32, stream: *mut c_void) {
        check(sys::phnsw_search_exact_labelset_device(self.ix, labels.lb, queries_dev, ldq, qids_dev, nq, exclude_dev,
                                                      want_first_dev, want_values_dev, nwant, k, out_ids_dev, out_d_dev,
                                                      out_len_dev, status_dev, stream));
    }

    /// `search_many_labeled` for a set of labels per query (`phnsw_search_batch_labelset`): the graph walk of query i
    /// restricted to the vectors `labels` lists under any label of `want[i]` -- the results `search_many_filtered` gives
    /// with the equivalent predicates, bit for bit.  A post-filter; `strict` also removes an entry vector whose label is
    /// not wanted.  The membership test is linear in the length of a set.  Panics unless `want` has one set per query
    pub fn search_many_labelset(&self, queries: &[Vec<f32>], sp: SearchParameters, labels: &GpuLabels, want: &[Vec<u32>],
                                strict: bool) -> Vec<Vec<(VectorId, f32)>> {
        let nq = queries.len();
        let (first, values) = pack_label_sets(want, nq, "search_many_labelset");
        let ef = sp.number_of_candidates;
        let psp = sp_c(sp);
        let mut q: Vec<f32> = Vec::with_capacity(nq * queries.first().map_or(0, |x| x.len()));
        for x in queries {
            q.extend_from_slice(x);
        }
        let (mut ids, mut d, mut len) = (vec![0u64; nq * ef], vec![0f32; nq * ef], vec![0u64; nq]);
        check(unsafe {
            sys::phnsw_search_batch_labelset(self.ix, labels.lb, q.as_ptr(), std::ptr::null(), nq as u64, &psp, 0, std::ptr::null(),
                                             first.as_ptr(), values.as_ptr(), if strict { 1 } else { 0 }, 0, ids.as_mut_ptr(),
                                             d.as_mut_ptr(), len.as_mut_ptr(), std::ptr::null_mut())
        });
        (0..nq).map(|i| (0..len[i] as usize).map(|j| (VectorId(ids[i * ef + j] as usize), d[i * ef + j])).collect()).collect()
    }

    /// zero-copy form (`phnsw_search_batch_labelset_device`): the sets in CSR form; status 8 = a range of
    /// `want_first_dev` that is not sound (that query does not walk); enqueued on `stream`, never synchronises it
    ///
    /// # Safety
    /// the pointers must be valid device allocations of the sizes `phnsw.h` documents for the call
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn search_batch_labelset_device(&self, labels: &GpuLabels, queries_dev: *const f32, ldq: u32,
                                               qids_dev: *const u32, nq: u64, sp: SearchParameters, upto_layers: u32,
                                               exclude_dev: *const u32, want_first_dev: *const u32,
                                               want_values_dev: *const u32, nwant: u64, flags: u32, out_ids_dev: *mut u32,
                                               out_d_dev: *mut f32, out_len_dev: *mut u32, out_stats_dev: *mut u32,
                                               status_dev: *mut u32, stream: *mut c_void) {
        let psp = sp_c(sp);
        check(sys::phnsw_search_batch_labelset_device(self.ix, labels.lb, queries_dev, ldq, qids_dev, nq, &psp, upto_layers,
                                                      exclude_dev, want_first_dev, want_values_dev, nwant, flags, out_ids_dev,
                                                      out_d_dev, out_len_dev, out_stats_dev, status_dev, stream));
    }

    /// `search_many_labeled_auto` for a set of labels per query (`phnsw_search_labelset_auto`): per query the scan by set
    /// or the strict walk by set, the scan again for short rows; every result holds min(k, candidates) entries, listed
    /// vectors of the labels of `want[i]` only.  `scan_below` 0 = the library's threshold for sets (20 000 rows of
    /// the union, `phnsw.h`), `u64::MAX` = always scan.  Returns the results and one route per query.  Panics
    /// unless 1 <= k <= number_of_candidates and `want` has one set per query
    pub fn search_many_labelset_auto(&self, queries: &[Vec<f32>], sp: SearchParameters, k: usize, scan_below: u64,
                                     labels: &GpuLabels, want: &[Vec<u32>]) -> (Vec<Vec<(VectorId, f32)>>, Vec<u32>) {
        assert!(k >= 1 && k <= sp.number_of_candidates, "search_many_labelset_auto: k must be 1..number_of_candidates");
        let nq = queries.len();
        let (first, values) = pack_label_sets(want, nq, "search_many_labelset_auto");
        let psp = sp_c(sp);
        let mut q: Vec<f32> = Vec::with_capacity(nq * queries.first().map_or(0, |x| x.len()));
        for x in queries {
            q.extend_from_slice(x);
        }
        let (mut ids, mut d, mut len) = (vec![0u64; nq * k], vec![0f32; nq * k], vec![0u64; nq]);
        let mut route = vec![0u32; nq];
        check(unsafe {
            sys::phnsw_search_labelset_auto(self.ix, labels.lb, q.as_ptr(), std::ptr::null(), nq as u64, &psp, std::ptr::null(),
                                            first.as_ptr(), values.as_ptr(), k as u64, scan_below, ids.as_mut_ptr(),
                                            d.as_mut_ptr(), len.as_mut_ptr(), route.as_mut_ptr())
        });
        let rows = (0..nq).map(|i| (0..len[i] as usize).map(|j| (VectorId(ids[i * k + j] as usize), d[i * k + j])).collect()).collect();
        (rows, route)
    }

    /// device form (`phnsw_search_labelset_auto_device`): u32 ids `[nq][k]`; synchronises `stream` up to twice
    ///
    /// # Safety
    /// the pointers must be valid device allocations of the sizes `phnsw.h` documents for the call
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn search_labelset_auto_device(&self, labels: &GpuLabels, queries_dev: *const f32, ldq: u32,
                                              qids_dev: *const u32, nq: u64, sp: SearchParameters, exclude_dev: *const u32,
                                              want_first_dev: *const u32, want_values_dev: *const u32, nwant: u64, k: u64,
                                              scan_below: u64, out_ids_dev: *mut u32, out_d_dev: *mut f32,
                                              out_len_dev: *mut u32, out_route_dev: *mut u32, status_dev: *mut u32,
                                              stream: *mut c_void) {
        let psp = sp_c(sp);
        check(sys::phnsw_search_labelset_auto_device(self.ix, labels.lb, queries_dev, ldq, qids_dev, nq, &psp, exclude_dev,
                                                     want_first_dev, want_values_dev, nwant, k, scan_below, out_ids_dev,
                                                     out_d_dev, out_len_dev, out_route_dev, status_dev, stream));
    }

    /// `search_many_filtered` by row label (`phnsw_search_batch_labeled`): the graph walk of query i restricted to the
    /// vectors `labels` lists under `want[i]`, read from the handle's label column instead of a bitmap per query -- the
    /// results `search_many_filtered` gives with the equivalent predicates, bit for bit.  A post-filter: about
    /// number_of_candidates * list length / N results; `strict` also removes an entry vector whose label differs.
    /// Panics unless `want` has one entry per query
    pub fn search_many_labeled(&self, queries: &[Vec<f32>], sp: SearchParameters, labels: &GpuLabels, want: &[Option<u32>],
                               strict: bool) -> Vec<Vec<(VectorId, f32)>> {
        let nq = queries.len();
        assert!(want.len() == nq, "search_many_labeled: one wanted label per query");
        let ef = sp.number_of_candidates;
        let psp = sp_c(sp);
        let w: Vec<u32> = want.iter().map(|l| l.unwrap_or(sys::PHNSW_LABEL_NONE)).collect();
        let mut q: Vec<f32> = Vec::with_capacity(nq * queries.first().map_or(0, |x| x.len()));
        for x in queries {
            q.extend_from_slice(x);
        }
        let (mut ids, mut d, mut len) = (vec![0u64; nq * ef], vec![0f32; nq * ef], vec![0u64; nq]);
        check(unsafe {
            sys::phnsw_search_batch_labeled(self.ix, labels.lb, q.as_ptr(), std::ptr::null(), nq as u64, &psp, 0, std::ptr::null(),
                                            w.as_ptr(), if strict { 1 } else { 0 }, 0, ids.as_mut_ptr(), d.as_mut_ptr(),
                                            len.as_mut_ptr(), std::ptr::null_mut())
        });
        (0..nq).map(|i| (0..len[i] as usize).map(|j| (VectorId(ids[i * ef + j] as usize), d[i * ef + j])).collect()).collect()
    }

    /// zero-copy form (`phnsw_search_batch_labeled_device`): rows of number_of_candidates u32 ids; enqueued on `stream`,
    /// never synchronises it
    ///
    /// # Safety
    /// the pointers must be valid device allocations of the sizes `phnsw.h` documents for the call
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn search_batch_labeled_device(&self, labels: &GpuLabels, queries_dev: *const f32, ldq: u32,
                                              qids_dev: *const u32, nq: u64, sp: SearchParameters, upto_layers: u32,
                                              exclude_dev: *const u32, want_dev: *const u32, flags: u32,
                                              out_ids_dev: *mut u32, out_d_dev: *mut f32, out_len_dev: *mut u32,
                                              out_stats_dev: *mut u32, status_dev: *mut u32, stream: *mut c_void) {
        let psp = sp_c(sp);
        check(sys::phnsw_search_batch_labeled_device(self.ix, labels.lb, queries_dev, ldq, qids_dev, nq, &psp, upto_layers,
                                                     exclude_dev, want_dev, flags, out_ids_dev, out_d_dev, out_len_dev,
                                                     out_stats_dev, status_dev, stream));
    }

    /// the collecting search (`phnsw_search_collect`): `search_many_topk` whose walk of the last layer also keeps the best
    /// `k` rows `include` accepts among those it evaluates, and returns them -- where `search_many_filtered` filters the
    /// queue afterwards.  `extend`: a hop that improved the kept rows counts as one that did something.  Panics unless
    /// 1 <= k <= 64 (k may exceed number_of_candidates)
    pub fn search_many_collect<F: Fn(VectorId) -> bool>(&self, queries: &[Vec<f32>], sp: SearchParameters, k: usize,
                                                        include: F, extend: bool) -> Vec<Vec<(VectorId, f32)>> {
        assert!(k >= 1 && k <= 64, "search_many_collect: k must be 1..64");
        let nq = queries.len();
        let psp = sp_c(sp);
        let mut n64 = 0u64;
        check(unsafe {
            sys::phnsw_store_info(self.comparator.store.0, &mut n64, std::ptr::null_mut(), std::ptr::null_mut(),
                                  std::ptr::null_mut(), std::ptr::null_mut())
        });
        let n = n64 as usize;
        let mut words = vec![0u32; (n + 31) / 32];
        for v in 0..n {
            if include(VectorId(v)) {
                words[v >> 5] |= 1u32 << (v & 31);
            }
        }
        let mut q: Vec<f32> = Vec::with_capacity(nq * queries.first().map_or(0, |x| x.len()));
        for x in queries {
            q.extend_from_slice(x);
        }
        let (mut ids, mut d, mut len) = (vec![0u64; nq * k], vec![0f32; nq * k], vec![0u64; nq]);
        check(unsafe {
            sys::phnsw_search_collect(self.ix, q.as_ptr(), std::ptr::null(), nq as u64, &psp, 0, std::ptr::null(), words.as_ptr(), 0,
                                      if extend { sys::PHNSW_COLLECT_EXTEND } else { 0 }, k as u64, ids.as_mut_ptr(),
                                      d.as_mut_ptr(), len.as_mut_ptr(), std::ptr::null_mut())
        });
        (0..nq).map(|i| (0..len[i] as usize).map(|j| (VectorId(ids[i * k + j] as usize), d[i * k + j])).collect()).collect()
    }

    /// zero-copy form (`phnsw_search_collect_device`): rows of `k` u32 ids; enqueued on `stream`, never synchronises it
    ///
    /// # Safety
    /// the pointers must be valid device allocations of the sizes `phnsw.h` documents for the call
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn search_collect_device(&self, queries_dev: *const f32, ldq: u32, qids_dev: *const u32, nq: u64,
                                        sp: SearchParameters, upto: u32, exclude_dev: *const u32, filter_dev: *const u32,
                                        filter_stride_words: u32, extend: bool, k: u64, out_ids_dev: *mut u32,
                                        out_d_dev: *mut f32, out_len_dev: *mut u32, out_stats_dev: *mut u32,
                                        status_dev: *mut u32, stream: *mut c_void) {
        let psp = sp_c(sp);
        check(sys::phnsw_search_collect_device(self.ix, queries_dev, ldq, qids_dev, nq, &psp, upto, exclude_dev, filter_dev,
                                               filter_stride_words, if extend { sys::PHNSW_COLLECT_EXTEND } else { 0 }, k,
                                               out_ids_dev, out_d_dev, out_len_dev, out_stats_dev, status_dev, stream));
    }

    /// `search_many_collect` by row label (`phnsw_search_collect_labeled`): the results `search_many_collect` gives with
    /// the equivalent predicates, bit for bit, read from the handle's label column.  Panics unless 1 <= k <= 64 and
    /// `want` has one entry per query
    pub fn search_many_collect_labeled(&self, queries: &[Vec<f32>], sp: SearchParameters, k: usize, labels: &GpuLabels,
                                       want: &[Option<u32>], extend: bool) -> Vec<Vec<(VectorId, f32)>> {
        assert!(k >= 1 && k <= 64, "search_many_collect_labeled: k must be 1..64");
        let nq = queries.len();
        assert!(want.len() == nq, "search_many_collect_labeled: one wanted label per query");
        let psp = sp_c(sp);
        let w: Vec<u32> = want.iter().map(|l| l.unwrap_or(sys::PHNSW_LABEL_NONE)).collect();
        let mut q: Vec<f32> = Vec::with_capacity(nq * queries.first().map_or(0, |x| x.len()));
        for x in queries {
            q.extend_from_slice(x);
        }
        let (mut ids, mut d, mut len) = (vec![0u64; nq * k], vec![0f32; nq * k], vec![0u64; nq]);
        check(unsafe {
            sys::phnsw_search_collect_labeled(self.ix, labels.lb, q.as_ptr(), std::ptr::null(), nq as u64, &psp, 0,
                                              std::ptr::null(), w.as_ptr(), if extend { sys::PHNSW_COLLECT_EXTEND } else { 0 },
                                              k as u64, ids.as_mut_ptr(), d.as_mut_ptr(), len.as_mut_ptr(), std::ptr::null_mut())
        });
        (0..nq).map(|i| (0..len[i] as usize).map(|j| (VectorId(ids[i * k + j] as usize), d[i * k + j])).collect()).collect()
    }

    /// zero-copy form (`phnsw_search_collect_labeled_device`): rows of `k` u32 ids; enqueued on `stream`, never
    /// synchronises it
    ///
    /// # Safety
    /// the pointers must be valid device allocations of the sizes `phnsw.h` documents for the call
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn search_collect_labeled_device(&self, labels: &GpuLabels, queries_dev: *const f32, ldq: u32,
                                                qids_dev: *const u32, nq: u64, sp: SearchParameters, upto_layers: u32,
                                                exclude_dev: *const u32, want_dev: *const u32, extend: bool, k: u64,
                                                out_ids_dev: *mut u32, out_d_dev: *mut f32, out_len_dev: *mut u32,
                                                out_stats_dev: *mut u32, status_dev: *mut u32, stream: *mut c_void) {
        let psp = sp_c(sp);
        check(sys::phnsw_search_collect_labeled_device(self.ix, labels.lb, queries_dev, ldq, qids_dev, nq, &psp, upto_layers,
                                                       exclude_dev, want_dev, if extend { sys::PHNSW_COLLECT_EXTEND } else { 0 },
                                                       k, out_ids_dev, out_d_dev, out_len_dev, out_stats_dev, status_dev, stream));
    }

    /// `search_many_filtered_auto` by row label (`phnsw_search_labeled_auto`): per query the posting-list scan or the
    /// strict walk by label, the scan again for short rows; every result holds min(k, list length) entries, listed
    /// vectors of `want[i]` only.  `scan_below` 0 = the library's threshold for labels (20 000, `phnsw.h`),
    /// `u64::MAX` = always scan.  Returns the results and one route per query.  Panics unless
    /// 1 <= k <= number_of_candidates and `want` has one entry per query
    pub fn search_many_labeled_auto(&self, queries: &[Vec<f32>], sp: SearchParameters, k: usize, scan_below: u64,
                                    labels: &GpuLabels, want: &[Option<u32>]) -> (Vec<Vec<(VectorId, f32)>>, Vec<u32>) {
        assert!(k >= 1 && k <= sp.number_of_candidates, "search_many_labeled_auto: k must be 1..number_of_candidates");
        let nq = queries.len();
        assert!(want.len() == nq, "search_many_labeled_auto: one wanted label per query");
        let psp = sp_c(sp);
        let w: Vec<u32> = want.iter().map(|l| l.unwrap_or(sys::PHNSW_LABEL_NONE)).collect();
        let mut q: Vec<f32> = Vec::with_capacity(nq * queries.first().map_or(0, |x| x.len()));
        for x in queries {
            q.extend_from_slice(x);
        }
        let (mut ids, mut d, mut len) = (vec![0u64; nq * k], vec![0f32; nq * k], vec![0u64; nq]);
        let mut route = vec![0u32; nq];
        check(unsafe {
            sys::phnsw_search_labeled_auto(self.ix, labels.lb, q.as_ptr(), std::ptr::null(), nq as u64, &psp, std::ptr::null(),
                                           w.as_ptr(), k as u64, scan_below, ids.as_mut_ptr(), d.as_mut_ptr(), len.as_mut_ptr(),
                                           route.as_mut_ptr())
        });
        let rows = (0..nq).map(|i| (0..len[i] as usize).map(|j| (VectorId(ids[i * k + j] as usize), d[i * k + j])).collect()).collect();
        (rows, route)
    }

    /// device form (`phnsw_search_labeled_auto_device`): u32 ids `[nq][k]`; synchronises `stream` up to twice
    ///
    /// # Safety
    /// the pointers must be valid device allocations of the sizes `phnsw.h` documents for the call
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn search_labeled_auto_device(&self, labels: &GpuLabels, queries_dev: *const f32, ldq: u32,
                                             qids_dev: *const u32, nq: u64, sp: SearchParameters, exclude_dev: *const u32,
                                             want_dev: *const u32, k: u64, scan_below: u64, out_ids_dev: *mut u32,
                                             out_d_dev: *mut f32, out_len_dev: *mut u32, out_route_dev: *mut u32,
                                             status_dev: *mut u32, stream: *mut c_void) {
        let psp = sp_c(sp);
        check(sys::phnsw_search_labeled_auto_device(self.ix, labels.lb, queries_dev, ldq, qids_dev, nq, &psp, exclude_dev,
                                                    want_dev, k, scan_below, out_ids_dev, out_d_dev, out_len_dev, out_route_dev,
                                                    status_dev, stream));
    }

    /// 0, or the code `search_many_exact_shared` would be refused with (`phnsw_exact_shared_supported`)
    pub fn exact_shared_supported(&self, k: usize) -> i32 {
        unsafe { sys::phnsw_exact_shared_supported(self.ix, k as u64) }
    }

    /// candidates of each of `nbitmaps` device bitmaps (`phnsw_filter_count_device`): what to choose between
    /// `search_many_filtered` and `search_many_exact_filtered` by
    ///
    /// # Safety
    /// `filter_dev` (or null: the default filter) and `out_count_dev` (`nbitmaps` u32) must be valid device allocations
    pub unsafe fn filter_count_device(&self, filter_dev: *const u32, filter_stride_words: u32, nbitmaps: u64,
                                      out_count_dev: *mut u32, stream: *mut c_void) {
        check(sys::phnsw_filter_count_device(self.ix, filter_dev, filter_stride_words, nbitmaps, out_count_dev, stream));
    }

    /// one filtered call that picks the scan or the graph walk per query and rescans what the walk left short
    /// (`phnsw_search_filtered_auto`): every result holds min(k, candidates) entries and only ids `include` accepts.
    /// `scan_below` 0 = the library's threshold, `u64::MAX` = always scan.  A graph-routed result is approximate
    /// (`phnsw.h`).  Returns the results and one route per query.  Panics unless 1 <= k <= number_of_candidates
    pub fn search_many_filtered_auto<F: Fn(VectorId) -> bool>(&self, queries: &[Vec<f32>], sp: SearchParameters, k: usize,
                                                              scan_below: u64, include: F)
                                                              -> (Vec<Vec<(VectorId, f32)>>, Vec<u32>) {
        assert!(k >= 1 && k <= sp.number_of_candidates, "search_many_filtered_auto: k must be 1..number_of_candidates");
        let psp = sp_c(sp);
        let nq = queries.len();
        let mut n64 = 0u64;
        check(unsafe {
            sys::phnsw_store_info(self.comparator.store.0, &mut n64, std::ptr::null_mut(), std::ptr::null_mut(),
                                  std::ptr::null_mut(), std::ptr::null_mut())
        });
        let n = n64 as usize;
        let mut words = vec![0u32; (n + 31) / 32];
        for v in 0..n {
            if include(VectorId(v)) {
                words[v >> 5] |= 1u32 << (v & 31);
            }
        }
        let mut q: Vec<f32> = Vec::with_capacity(nq * queries.first().map_or(0, |x| x.len()));
        for x in queries {
            q.extend_from_slice(x);
        }
        let (mut ids, mut d, mut len) = (vec![0u64; nq * k], vec![0f32; nq * k], vec![0u64; nq]);
        let mut route = vec![0u32; nq];
        check(unsafe {
            sys::phnsw_search_filtered_auto(self.ix, q.as_ptr(), std::ptr::null(), nq as u64, &psp, std::ptr::null(), words.as_ptr(),
                                            0, k as u64, scan_below, ids.as_mut_ptr(), d.as_mut_ptr(), len.as_mut_ptr(),
                                            route.as_mut_ptr())
        });
        let rows = (0..nq).map(|i| (0..len[i] as usize).map(|j| (VectorId(ids[i * k + j] as usize), d[i * k + j])).collect()).collect();
        (rows, route)
    }

    /// device form (`phnsw_search_filtered_auto_device`): u32 ids `[nq][k]`; synchronises `stream` up to twice
    ///
    /// # Safety
    /// the pointers must be valid device allocations of the sizes `phnsw.h` documents for the call
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn search_filtered_auto_device(&self, queries_dev: *const f32, ldq: u32, qids_dev: *const u32, nq: u64,
                                              sp: SearchParameters, exclude_dev: *const u32, filter_dev: *const u32,
                                              filter_stride_words: u32, k: u64, scan_below: u64, out_ids_dev: *mut u32,
                                              out_d_dev: *mut f32, out_len_dev: *mut u32, out_route_dev: *mut u32,
                                              status_dev: *mut u32, stream: *mut c_void) {
        let psp = sp_c(sp);
        check(sys::phnsw_search_filtered_auto_device(self.ix, queries_dev, ldq, qids_dev, nq, &psp, exclude_dev, filter_dev,
                                                     filter_stride_words, k, scan_below, out_ids_dev, out_d_dev, out_len_dev,
                                                     out_route_dev, status_dev, stream));
    }

    /// an index over a `to_f16()` comparator: search it, recompute every result's distance on the f32 comparator
    /// `full`, sort by (distance, id), keep the best `k` (`phnsw_f16_search_batch`)
    pub fn search_many_reranked(&self, full: &GpuComparator, queries: &[Vec<f32>], sp: SearchParameters, k: usize)
                                -> Vec<Vec<(VectorId, f32)>> {
        let nq = queries.len();
        let psp = sp_c(sp);
        let mut q: Vec<f32> = Vec::with_capacity(nq * queries.first().map_or(0, |x| x.len()));
        for x in queries {
            q.extend_from_slice(x);
        }
        let (mut ids, mut d, mut len) = (vec![0u64; nq * k], vec![0f32; nq * k], vec![0u64; nq]);
        check(unsafe {
            sys::phnsw_f16_search_batch(self.ix, full.store.0, q.as_ptr(), nq as u64, &psp, k as u64, ids.as_mut_ptr(),
                                        d.as_mut_ptr(), len.as_mut_ptr())
        });
        (0..nq).map(|i| (0..len[i] as usize).map(|j| (VectorId(ids[i * k + j] as usize), d[i * k + j])).collect()).collect()
    }

    /// `search_many_reranked` for an index over a `to_i8()` comparator (`phnsw_i8_search_batch`)
    pub fn search_many_reranked_i8(&self, full: &GpuComparator, queries: &[Vec<f32>], sp: SearchParameters, k: usize)
                                   -> Vec<Vec<(VectorId, f32)>> {
        let nq = queries.len();
        let psp = sp_c(sp);
        let mut q: Vec<f32> = Vec::with_capacity(nq * queries.first().map_or(0, |x| x.len()));
        for x in queries {
            q.extend_from_slice(x);
        }
        let (mut ids, mut d, mut len) = (vec![0u64; nq * k], vec![0f32; nq * k], vec![0u64; nq]);
        check(unsafe {
            sys::phnsw_i8_search_batch(self.ix, full.store.0, q.as_ptr(), nq as u64, &psp, k as u64, ids.as_mut_ptr(),
                                       d.as_mut_ptr(), len.as_mut_ptr())
        });
        (0..nq).map(|i| (0..len[i] as usize).map(|j| (VectorId(ids[i * k + j] as usize), d[i * k + j])).collect()).collect()
    }

    /// zero-copy form (`phnsw_i8_search_batch_device`): every pointer is device memory of the caller, the work is
    /// enqueued on `stream` without synchronisation; rows keep the stride `sp.number_of_candidates`
    ///
    /// # Safety
    /// the pointers must be valid device allocations of the sizes `phnsw.h` documents for the call
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn search_reranked_i8_device(&self, full: &GpuComparator, queries_dev: *const f32, ldq: u32, nq: u64,
                                            sp: SearchParameters, k: u64, out_ids_dev: *mut u32, out_d_dev: *mut f32,
                                            out_len_dev: *mut u32, out_stats_dev: *mut u32, status_dev: *mut u32,
                                            stream: *mut c_void) {
        let psp = sp_c(sp);
        check(sys::phnsw_i8_search_batch_device(self.ix, full.store.0, queries_dev, ldq, nq, &psp, k, out_ids_dev, out_d_dev,
                                                out_len_dev, out_stats_dev, status_dev, stream));
    }

    /// `search_many_reranked` for an index over a `to_i8q()` comparator (`phnsw_i8q_search_batch`)
    pub fn search_many_reranked_i8q(&self, full: &GpuComparator, queries: &[Vec<f32>], sp: SearchParameters, k: usize)
                                    -> Vec<Vec<(VectorId, f32)>> {
        let nq = queries.len();
        let psp = sp_c(sp);
        let mut q: Vec<f32> = Vec::with_capacity(nq * queries.first().map_or(0, |x| x.len()));
        for x in queries {
            q.extend_from_slice(x);
        }
        let (mut ids, mut d, mut len) = (vec![0u64; nq * k], vec![0f32; nq * k], vec![0u64; nq]);
        check(unsafe {
            sys::phnsw_i8q_search_batch(self.ix, full.store.0, q.as_ptr(), nq as u64, &psp, k as u64, ids.as_mut_ptr(),
                                        d.as_mut_ptr(), len.as_mut_ptr())
        });
        (0..nq).map(|i| (0..len[i] as usize).map(|j| (VectorId(ids[i * k + j] as usize), d[i * k + j])).collect()).collect()
    }

    /// zero-copy form (`phnsw_i8q_search_batch_device`), as `search_reranked_i8_device`
    ///
    /// # Safety
    /// the pointers must be valid device allocations of the sizes `phnsw.h` documents for the call
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn search_reranked_i8q_device(&self, full: &GpuComparator, queries_dev: *const f32, ldq: u32, nq: u64,
                                             sp: SearchParameters, k: u64, out_ids_dev: *mut u32, out_d_dev: *mut f32,
                                             out_len_dev: *mut u32, out_stats_dev: *mut u32, status_dev: *mut u32,
                                             stream: *mut c_void) {
        let psp = sp_c(sp);
        check(sys::phnsw_i8q_search_batch_device(self.ix, full.store.0, queries_dev, ldq, nq, &psp, k, out_ids_dev, out_d_dev,
                                                 out_len_dev, out_stats_dev, status_dev, stream));
    }

    /// `search_many_reranked` for an index over a `to_bits()` comparator (`phnsw_bits_search_batch`): the walk runs on
    /// Hamming distances, the returned distances are true f32 distances on `full`
    pub fn search_many_reranked_bits(&self, full: &GpuComparator, queries: &[Vec<f32>], sp: SearchParameters, k: usize)
                                     -> Vec<Vec<(VectorId, f32)>> {
        let nq = queries.len();
        let psp = sp_c(sp);
        let mut q: Vec<f32> = Vec::with_capacity(nq * queries.first().map_or(0, |x| x.len()));
        for x in queries {
            q.extend_from_slice(x);
        }
        let (mut ids, mut d, mut len) = (vec![0u64; nq * k], vec![0f32; nq * k], vec![0u64; nq]);
        check(unsafe {
            sys::phnsw_bits_search_batch(self.ix, full.store.0, q.as_ptr(), nq as u64, &psp, k as u64, ids.as_mut_ptr(),
                                         d.as_mut_ptr(), len.as_mut_ptr())
        });
        (0..nq).map(|i| (0..len[i] as usize).map(|j| (VectorId(ids[i * k + j] as usize), d[i * k + j])).collect()).collect()
    }

    /// zero-copy form (`phnsw_bits_search_batch_device`), as `search_reranked_i8_device`
    ///
    /// # Safety
    /// the pointers must be valid device allocations of the sizes `phnsw.h` documents for the call
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn search_reranked_bits_device(&self, full: &GpuComparator, queries_dev: *const f32, ldq: u32, nq: u64,
                                              sp: SearchParameters, k: u64, out_ids_dev: *mut u32, out_d_dev: *mut f32,
                                              out_len_dev: *mut u32, out_stats_dev: *mut u32, status_dev: *mut u32,
                                              stream: *mut c_void) {
        let psp = sp_c(sp);
        check(sys::phnsw_bits_search_batch_device(self.ix, full.store.0, queries_dev, ldq, nq, &psp, k, out_ids_dev, out_d_dev,
                                                  out_len_dev, out_stats_dev, status_dev, stream));
    }

    /// `Hnsw::search_instrumented(v, sp)`  lib.rs:667-673
    pub fn search_instrumented(&self, v: AbstractVector<Vec<f32>>, sp: SearchParameters) -> (Vec<(VectorId, f32)>, usize) {
        let ef = sp.number_of_candidates;
        let psp = sp_c(sp);
        let (mut ids, mut d, mut len, mut index) = (vec![0u64; ef], vec![0f32; ef], 0u64, 0u64);
        let rc = match &v {
            AbstractVector::Stored(i) => {
                let q = i.0 as u64;
                unsafe {
                    sys::phnsw_search_instrumented(self.ix, std::ptr::null(), &q, 1, &psp, ids.as_mut_ptr(), d.as_mut_ptr(),
                                                   &mut len, &mut index)
                }
            }
            AbstractVector::Unstored(x) => unsafe {
                sys::phnsw_search_instrumented(self.ix, x.as_ptr(), std::ptr::null(), 1, &psp, ids.as_mut_ptr(),
                                               d.as_mut_ptr(), &mut len, &mut index)
            },
        };
        check(rc);
        ((0..len as usize).map(|j| (VectorId(ids[j] as usize), d[j])).collect(), index as usize) // u64::MAX == usize::MAX
    }

    /// `Hnsw::improve_index(bp, last_recall, progress)`  lib.rs:1664-1669
    pub fn improve_index(&mut self, bp: BuildParameters, last_recall: Option<f32>,
                         progress: &mut dyn ProgressMonitor) -> f32 {
        let mut out = 0f32;
        let mut monitor: &mut dyn ProgressMonitor = progress;
        check(unsafe {
            sys::phnsw_improve_index(self.ix, &bp_c(bp, 0), last_recall.unwrap_or(f32::NAN), Some(progress_trampoline),
                                     &mut monitor as *mut &mut dyn ProgressMonitor as *mut c_void, &mut out)
        });
        out
    }
    /// `Hnsw::improve_neighbors(op, last_recall)`  lib.rs:1507-1513
    pub fn improve_neighbors(&mut self, op: OptimizationParameters, last_recall: Option<f32>) -> f32 {
        let mut bp = self.build_parameters;
        bp.optimization = op;
        let mut out = 0f32;
        check(unsafe {
            sys::phnsw_improve_neighbors_upto(self.ix, self.layer_count() as u32, &bp_c(bp, 0),
                                              last_recall.unwrap_or(f32::NAN), &mut out)
        });
        out
    }
    /// `Hnsw::stochastic_recall(op)`  lib.rs:1501-1505
    pub fn stochastic_recall(&self, op: OptimizationParameters) -> f32 {
        let mut out = 0f32;
        check(unsafe { sys::phnsw_stochastic_recall_at(self.ix, self.layer_count() as u32 - 1, &op_c(op), &mut out) });
        out
    }

    /// `Hnsw::knn(k, probe_depth)`  lib.rs:905-928 (collected: one launch over the bottom layer)
    pub fn knn(&self, k: usize, probe_depth: usize) -> Vec<(VectorId, Vec<(VectorId, f32)>)> {
        let n = self.vector_count();
        let (mut ids, mut d, mut len) = (vec![0u64; n * k], vec![0f32; n * k], vec![0u64; n]);
        check(unsafe {
            sys::phnsw_knn(self.ix, k as u64, probe_depth as u64, ids.as_mut_ptr(), d.as_mut_ptr(), len.as_mut_ptr())
        });
        self.pair_up(&ids, &d, &len, k)
    }
    /// `Hnsw::threshold_nn(threshold, probe_depth, initial_search_depth)`  lib.rs:930-962
    pub fn threshold_nn(&self, threshold: f32, probe_depth: usize, initial_search_depth: usize, max_out: usize)
                        -> Vec<(VectorId, Vec<(VectorId, f32)>)> {
        let n = self.vector_count();
        let (mut ids, mut d, mut len) = (vec![0u64; n * max_out], vec![0f32; n * max_out], vec![0u64; n]);
        check(unsafe {
            sys::phnsw_threshold_nn(self.ix, threshold, probe_depth as u64, initial_search_depth as u64,
                                    max_out as u64, ids.as_mut_ptr(), d.as_mut_ptr(), len.as_mut_ptr())
        });
        self.pair_up(&ids, &d, &len, max_out)
    }
    fn pair_up(&self, ids: &[u64], d: &[f32], len: &[u64], stride: usize) -> Vec<(VectorId, Vec<(VectorId, f32)>)> {
        let bottom = self.layer(self.layer_count() - 1);
        bottom.nodes.iter().enumerate().map(|(i, v)| {
            (*v, (0..len[i] as usize).map(|j| (VectorId(ids[i * stride + j] as usize), d[i * stride + j])).collect())
        }).collect()
    }

    /// the crate's directory format (serialize.rs:33-209), written / read by libphnsw itself
    pub fn serialize<P: AsRef<Path>>(&self, path: P) {
        let p = CString::new(path.as_ref().to_str().expect("utf-8 path")).unwrap();
        check(unsafe { sys::phnsw_index_serialize(self.ix, p.as_ptr()) });
    }
    pub fn deserialize<P: AsRef<Path>>(path: P, c: GpuComparator) -> Self {
        let p = CString::new(path.as_ref().to_str().expect("utf-8 path")).unwrap();
        let mut ix = std::ptr::null_mut();
        check(unsafe { sys::phnsw_index_deserialize(c.store.0, p.as_ptr(), &mut ix) });
        let mut bp = std::mem::MaybeUninit::<sys::phnsw_build_params>::uninit();
        check(unsafe { sys::phnsw_index_build_params(ix, bp.as_mut_ptr()) });
        let b = unsafe { bp.assume_init() };
        let sp = |s: sys::phnsw_search_params| SearchParameters {
            number_of_candidates: s.number_of_candidates as usize,
            upper_layer_candidate_count: s.upper_layer_candidate_count as usize,
            probe_depth: s.probe_depth as usize,
        };
        let build_parameters = BuildParameters {
            order: b.order as usize,
            zero_layer_neighborhood_size: b.zero_layer_neighborhood_size as usize,
            neighborhood_size: b.neighborhood_size as usize,
            optimization: OptimizationParameters {
                promotion_threshold: b.optimization.promotion_threshold,
                neighborhood_threshold: b.optimization.neighborhood_threshold,
                recall_proportion: b.optimization.recall_proportion,
                promotion_proportion: b.optimization.promotion_proportion,
                search: sp(b.optimization.search),
            },
            initial_partition_search: sp(b.initial_partition_search),
        };
        GpuHnsw { ix, comparator: c, build_parameters }
    }
}
