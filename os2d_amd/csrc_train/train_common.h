// Shared by the translation units of libos2d_train.so: the error text that os2d_train_last_error() returns lives in train.hip.
#ifndef OS2D_TRAIN_COMMON_H
#define OS2D_TRAIN_COMMON_H

// Stores `text` as the calling thread's last error (not exported).
__attribute__((visibility("hidden"))) void os2d_train_store_error(const char* text);

#endif
