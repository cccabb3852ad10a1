// hip_stub.h -- TEST INFRASTRUCTURE: the books of tests/host/hip_stub.cpp as the harnesses read them.  The stub includes this header
// itself, so a signature that drifts from its definition does not compile.
#pragma once

extern "C" {
long hipstub_launches();
long hipstub_launches_on(void* stream);           // (NULL: the null stream)
long hipstub_launches_of(const char* name_part);  // launches of the kernels whose registered (mangled) name contains name_part
long hipstub_bad_waits();                         // hipStreamWaitEvent / hipEventSynchronize on an event never recorded
long hipstub_bad_launches();                      // a launch with a zero / oversized configuration or a dead stream
long hipstub_live_allocs();
long hipstub_live_streams();
long hipstub_live_events();
long hipstub_mallocs();
long hipstub_work_on_device(int d);
long hipstub_wrong_device();                      // a launch / record / copy that touched another device's stream, event or memory
void hipstub_fail_malloc_at(long nth);            // the nth hipMalloc FROM NOW (1 = the next) fails once; -1: never
void hipstub_set_devices(int n);
void hipstub_trace_begin();                       // forget the trace so far and record from here
long hipstub_trace_end();                         // stop recording; -> records held (read with hipstub_trace_record until the next begin)
const char* hipstub_trace_record(long i);
}
